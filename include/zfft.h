/*
 * zfft.h -- C-ABI of the MI355X Zoom-FFT spectrum/waterfall engine (libzfft.so).
 *
 * Drop-in boundary for pypanadapter's IQ -> waterfall-line hot path.  The reference has
 * no FFI: the path is inline numpy/scipy.  Each entry point below replaces a reference
 * call site (file:line under alfille/pypanadapter):
 *
 *   zfft_process        ApplicationDisplay.update (pypanadapter_spectrum.py:2102-2119):
 *                       zoomfft -> welch -> fftshift/crop -> 20*log10, one row per frame;
 *                       PSD.update (pypanadapter_thread.py:1513-1548), threaded caller.
 *   zfft_decimate       ApplicationDisplay.zoomfft (pypanadapter_spectrum.py:2088-2100).
 *   zfft_waterfall_*    Waterfall.init_image / image_update (pypanadapter_spectrum.py:
 *                       1625-1664), kept as a device ring + offset instead of np.roll.
 *   zfft_waterfall_reset ApplicationDisplay.on_invertscroll_clicked (S:2074-2077).
 *
 * Conventions: IQ is interleaved float32 (complex64, numpy's layout).  Rows are float32,
 * length n_win, dB = 20*log10(PSD) exactly as the reference computes it.  Every function
 * returns 0 on success or a negative ZFFT_E* code; zfft_last_error() (thread-local)
 * holds the message.  A plan is not re-entrant: one plan per calling thread; plans on
 * different devices run concurrently.  The caller owns all host buffers; the plan owns
 * its device buffers, HIP stream and tables.
 */
#ifndef ZFFT_H
#define ZFFT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZFFT_VERSION 1

/* error codes */
#define ZFFT_OK 0
#define ZFFT_EINVAL (-1)       /* bad argument / config (ValueError in the Python shim) */
#define ZFFT_ESHORT (-2)       /* frame too short: a decimation stage has <= 27 samples  */
#define ZFFT_EHIP (-3)         /* HIP runtime failure                                    */
#define ZFFT_ENOMEM (-4)       /* device or host allocation failed                       */
#define ZFFT_ENODEV (-5)       /* no HIP device                                          */
#define ZFFT_EUNSUPPORTED (-6) /* valid in the reference but not built in this version   */
#define ZFFT_EINTERNAL (-7)    /* the library's own filter tables failed a consistency check */

/* window kinds: scipy.signal.get_window(kind, M) with fftbins=True (periodic), the taper
 * list of FFTTaperingControl (pypanadapter_spectrum.py:1222-1243) */
enum zfft_window_kind {
  ZFFT_WIN_HAMMING = 0, /* AppState.fft_tapering default, S:1492 */
  ZFFT_WIN_HANN = 1,
  ZFFT_WIN_BLACKMAN = 2,
  ZFFT_WIN_BLACKMANHARRIS = 3,
  ZFFT_WIN_NUTTALL = 4,
  ZFFT_WIN_FLATTOP = 5,
  ZFFT_WIN_BARTHANN = 6,
  ZFFT_WIN_BARTLETT = 7,
  ZFFT_WIN_TRIANG = 8,
  ZFFT_WIN_BOHMAN = 9,
  ZFFT_WIN_PARZEN = 10,
  ZFFT_WIN_BOXCAR = 11,
  ZFFT_WIN_KAISER = 12,           /* window_param[0] = beta              */
  ZFFT_WIN_GAUSSIAN = 13,         /* window_param[0] = std               */
  ZFFT_WIN_GENERAL_GAUSSIAN = 14, /* window_param = {p, sig}              */
  ZFFT_WIN_TUKEY = 15,            /* window_param[0] = alpha (NaN: 0.5)  */
  ZFFT_WIN_EXPONENTIAL = 16,      /* window_param = {center, tau}; NaN = scipy default
                                     (get_window(('exponential', 3), N) binds 3 to center) */
  ZFFT_WIN_CHEBWIN = 17,          /* window_param[0] = attenuation, dB   */
  ZFFT_WIN_DPSS = 18,             /* window_param[0] = NW (single taper)  */
  ZFFT_WIN_ARRAY = 100            /* caller-supplied float window (any scipy window) */
};

typedef struct zfft_config {
  int32_t n_fft;           /* N: power of two, 32..65536 (AppState.fft_size, S:1397; cfg5)  */
  int32_t zoom;            /* power of two, 1..512 (AppState.fft_ratio, S:2079-2086)        */
  int32_t n_win;           /* W: row stride, 2..N (N_WIN S:1757; T:1542); odd W gives the
                              reference's W - 1 entries (zfft_plan_row_length)            */
  int32_t window_kind;     /* enum zfft_window_kind                                         */
  double fs;               /* sample rate, Hz (panadapter.SampleRate)                       */
  double f_lo;             /* LO frequency, Hz; the reference hard-codes 1.0 (S:2090)       */
  double window_param[2];  /* see window kinds; NaN = parameter absent (scipy's default)      */
  int32_t scroll;          /* waterfall direction, +1 or -1 (AppState.scroll, S:1496)       */
  int32_t in_dtype;        /* 0 = complex64 (interleaved f32, 8 B/sample); 1 = complex32
                              (interleaved f16, 4 B/sample, BASELINE cfg5); 2 = RTL-SDR
                              interleaved uint8 I,Q (2 B/sample), value b/127.5 - 1 as
                              pyrtlsdr's packed_bytes_to_iq; 3 = real f32
                              (4 B/sample: AudioPan's paFloat32 stream, S:712-713, §8f-4)  */
  int32_t device;          /* HIP device ordinal                                            */
  int32_t flip_input;      /* 1 = reverse each frame on load: the np.flip the RTL-SDR
                              sources apply (S:541-543, 459-460), fused into stage 0       */
} zfft_config;

typedef struct zfft_plan zfft_plan;

/* Create a plan.  window_or_null: with ZFFT_WIN_ARRAY, a float window of length n_fft (the
 * array welch receives; frames whose decimated length is < n_fft are then rejected, as
 * scipy rejects a window longer than the input). */
int zfft_plan_create(const zfft_config *cfg, const float *window_or_null, zfft_plan **out);
int zfft_plan_destroy(zfft_plan *plan);
int zfft_plan_config(const zfft_plan *plan, zfft_config *out);  /* the configuration in use */
/* Valid floats per row (rows keep the stride n_win): the length of the reference's slice
 * fftshift(P)[N//2 - W//2 : N//2 + W//2] (S:2114), i.e. n_win rounded down to even, except
 * for real input (in_dtype 3) at zoom 1, where the reference's welch is one-sided and that
 * slice of the N/2+1 bins is shorter.  A waterfall of any width >= 40/60
 * (the one-sided rows are odd) is a plan with n_win = that width. */
int zfft_plan_row_length(const zfft_plan *plan);

/* Host-buffer path: n_frames frames of n_samples IQ each (frame-major), rows_out holds
 * n_frames*n_win floats.  Synchronous.  PCIe-inclusive. */
int zfft_process(zfft_plan *plan, const void *iq, int64_t n_samples, int32_t n_frames,
                 float *rows_out);

/* Device-buffer path: d_iq and d_rows are device pointers on the plan's device.  Enqueued
 * on `hip_stream` (a hipStream_t; NULL = HIP's default stream); returns without syncing. */
int zfft_process_device(zfft_plan *plan, const void *d_iq, int64_t n_samples, int32_t n_frames,
                        float *d_rows, void *hip_stream);

/* zoomfft (S:2088-2100): LO mix then log2(zoom) x decimate(x, 2).  out_iq receives
 * zfft_decimated_length(n_samples, zoom) complex64 samples.  Synchronous, host buffers. */
int zfft_decimate(zfft_plan *plan, const void *iq, int64_t n_samples, void *out_iq,
                  int64_t *out_len);
/* The same for n_frames frames in one call (frame-major, as zfft_process takes them), on the
 * schedule that many frames earn: out_iq receives n_frames x zfft_decimated_length complex64,
 * frame-major; out_len the length per frame. */
int zfft_decimate_frames(zfft_plan *plan, const void *iq, int64_t n_samples, int32_t n_frames,
                         void *out_iq, int64_t *out_len);
int64_t zfft_decimated_length(int64_t n_samples, int32_t zoom);

/* Waterfall ring: H = n_win/4 rows of n_win floats, reference row order on read. */
int zfft_waterfall_push(zfft_plan *plan, const float *row /* host, n_win; NULL = last row of
                                                             the last zfft_process* frame:
                                                             ZFFT_EINVAL when the plan's rows
                                                             are shorter than n_win */);
/* d_rows: count rows of n_win floats, every column defined (a row shorter than n_win --
 * zfft_plan_row_length < n_win -- leaves its tail columns unwritten: pad them first). */
int zfft_waterfall_push_device(zfft_plan *plan, const float *d_rows, int32_t count,
                               void *hip_stream);
int zfft_waterfall_read(zfft_plan *plan, float *img_out /* host, H*n_win */);
int zfft_waterfall_reset(zfft_plan *plan, int32_t scroll);
int zfft_waterfall_shape(const zfft_plan *plan, int32_t *rows, int32_t *cols);

/* Host IQ accumulation ring: pypanadapter_thread.py's `Data` (T:1400-1483)
 * between the reader thread and the PSD worker, in pinned host memory.  capacity =
 * 16 * chunk_size (T:1409); zfft_ring_add = Data.add without the pacing sleep: a chunk that
 * would run past the end is written at 0 instead (T:1437-1442), real_size is the high-water
 * mark and total_size the samples added since the last drain; zfft_ring_take =
 * get_data_start / data[:real_size] / get_data_end (T:1516-1520): it returns that frame
 * (after a fold-back: newest chunks first, as the reference reads it) and resets the
 * counts.  Two buffers alternate, so the returned frame stays intact until the next take
 * while add() continues (the reference's consumer keeps a view the reader may overwrite).
 * zfft_ring_process = PSD.update (T:1513-1548): take, skip frames shorter than n_fft
 * (*produced = 0), else one row through zfft_process from the pinned frame.  Thread-safe:
 * one producer and one consumer. */
typedef struct zfft_ring zfft_ring;
int zfft_ring_create(int64_t chunk_size, int32_t in_dtype, zfft_ring **out);
int zfft_ring_destroy(zfft_ring *ring);
int zfft_ring_add(zfft_ring *ring, const void *chunk, int64_t n_samples);
int zfft_ring_state(zfft_ring *ring, int64_t *size, int64_t *real_size, int64_t *total_size);
int zfft_ring_take(zfft_ring *ring, const void **frame, int64_t *n_samples, int64_t *total_size);
int zfft_ring_process(zfft_ring *ring, zfft_plan *plan, float *row_out /* host, n_win */,
                      int32_t *produced);

/* On-device waterfall rendering.  The reference hands img_array.T to a
 * pyqtgraph ImageItem with a 256-entry colormap LUT and fixed levels (Waterfall.__init__ /
 * lookuptable / newlevel / autolevel, pypanadapter_spectrum.py:1579-1623, 1667-1685); these
 * produce the RGBA pixels that ImageItem draws for the ring image, on the device:
 *   pixel = LUT[clip(trunc((v - min) * 256 / (max - min)), 0, 255)], alpha 255
 * (pyqtgraph makeARGB / rescaleData / applyLookupTable), rows in zfft_waterfall_read order.
 * Colormaps 'Default', 'Matrix', 'Red Green', 'Tropical' (S:1580-1585; any other name ->
 * 'Default', S:1613-1616); the LUT is linspace(0, 1, 256) through the stops, channels
 * truncated to uint8 (ColorMap.getLookupTable(0, 1, 256)).  'Default' carries the
 * reference's out-of-range stop value 2020 as numpy < 2 stored it in a uint8 (2020 mod 256
 * = 228; numpy 2 raises OverflowError there).  Initial levels -220 .. -120 (S:1593-1598).
 * autolevel sets the levels to the 2nd and 98th percentiles (numpy 'linear') of the pixels
 * below 0 -- what S:1676 computes; the reference then assigns them to unused attributes,
 * so its autolevel never changes the levels (a bug, SURVEY §8 a-6 note). */
int zfft_colormap_lut(const char *name, uint8_t *lut_rgba /* 256*4; no plan, no GPU */);
int zfft_waterfall_colormap(zfft_plan *plan, const char *name);
int zfft_waterfall_levels(zfft_plan *plan, double minlev, double maxlev);
int zfft_waterfall_get_levels(const zfft_plan *plan, double *minlev, double *maxlev);
int zfft_waterfall_autolevel(zfft_plan *plan, double *minlev, double *maxlev);
int zfft_waterfall_render(zfft_plan *plan, uint8_t *rgba_out /* host, H*n_win*4 */);
int zfft_waterfall_render_device(zfft_plan *plan, uint8_t *d_rgba /* H*n_win*4 */,
                                 void *hip_stream);
/* The per-line display in one round trip (Waterfall.image_update then the image the Qt side
 * draws, S:1638-1664): `count` host rows of n_win floats pushed as zfft_waterfall_push would
 * (0 = none), then the image emitted -- RGBA8 as zfft_waterfall_render, or float64 as the
 * reference's img_array (zfft_waterfall_read's floats widened) -- and copied to the host, with
 * one kernel for a single row, one copy and one wait (the rows are staged in page-locked
 * memory the kernel reads in place).  Same ring and image as the separate calls. */
int zfft_waterfall_push_render(zfft_plan *plan, const float *rows, int32_t count,
                               uint8_t *rgba_out /* host, H*n_win*4 */);
int zfft_waterfall_push_read64(zfft_plan *plan, const float *rows, int32_t count,
                               double *img_out /* host, H*n_win */);

/* Page-locked host memory (hipHostMalloc on the current device), e.g. for rgba_out: a render
 * (or a zfft_process row block) copied into it moves at PCIe DMA rate; into pageable memory
 * the runtime stages the copy through its own bounce buffer at a fraction of that (W = 8192:
 * 67 MB per image).  Free with zfft_host_free. */
int zfft_host_alloc(size_t bytes, void **out);
int zfft_host_free(void *ptr);

/* Native window generation (fp64), for tests and for callers without scipy. */
int zfft_window_values(int32_t kind, const double *param, int32_t length, double *out);

/* Block size / warm-up of the device decimator (0 = automatic).  Diagnostics. */
int zfft_plan_tune(zfft_plan *plan, int32_t block, int32_t warmup);

/* Per-launch HIP-event timing of zfft_process*: when enabled, the plan brackets every
 * kernel it launches with events on the launch stream; zfft_plan_timings then returns the
 * durations (ms) of the last call, in launch order, named by zfft_plan_timing_names: per
 * decimation stage one "xa_stage_mix"/"xa_stage" interval (XA schedule) or a forward and a
 * backward pass (blocked schedules), then the Welch kernel ("welch_rows" / "welch4").  A
 * batched zfft_process call reports every batch ("batch_wait" = the gap before batch k >= 1,
 * mostly its H2D copy).  Diagnostics; adds event records. */
int zfft_plan_timing(zfft_plan *plan, int32_t enable);
int zfft_plan_timings(zfft_plan *plan, float *ms_out, int32_t max, int32_t *count);
/* Comma-separated names of the intervals zfft_plan_timings returns (owned by the plan). */
const char *zfft_plan_timing_names(zfft_plan *plan);

/* Decimator schedule (path 0 ... 7): 0 = automatic -- for zoom 8 and frames of >= 16384 samples 4 below
 * 16 frames per call and 6 from there (zoom >= 16: the same for the first three stages;
 * zoom 4: 4 below 32 frames per call and 6 from there; zoom 2: 4 below 512); otherwise 3 for
 * batches of >= 768 frames, or >= 384 frames of <= 2^19
 * samples, else 2 for batches of >= 2^27 samples whose frames are long enough for the edge
 * windows, else 1 -- e.g. one frame per call, the reference's use.  Each batch of a
 * zfft_process call is judged by its own frame count (host calls are split into batches of
 * about 1 GiB of input -- 418 cfg2 frames); crossovers measured by tools/sweep_schedule.py,
 * tools/sweep_walk.py and tools/fc_ab.py (profiles/r04v, r06k, r06fc).  Default tolerance:
 * path 6 gives the float64 reference's decimated IQ within 6.5e-7 of its peak for content the
 * filter passes (measured worst 6.0e-7 on noise plus in-band tones, tests/test_gpu_fc.py FC_TOL).
 * FC applies the response truncated at |k| <= K, a coherent error on top of that: for a carrier
 * near the last stage's cutoff up to 1.09e-6 of the carrier at 1.04 x the cutoff at zoom 8
 * (7.7e-7 of it, times the LO's sqrt 2), 2.4e-8 at zoom 4 and 2.4e-8 at zoom 2 (path 7), 1.8e-7
 * at zoom 16; for a carrier in the stopband <= 7e-8 (the float64 models of
 * tests/dynrange_ref.py trunc_term, recorded per case in tests/golden/dynrange.json).  On every
 * path the error scales with the strongest input component, wherever it lies -- not with the
 * displayed content: a full-scale carrier outside the band leaves an error floor of 1e-7 ... 4e-7
 * of the carrier on FC and PC (-128 dBc and below), 2e-6 on paths 1 and 2, 1e-5 on XA under in-band
 * content that may be 100 dB weaker (tests/test_gpu_dynrange.py).  The constants
 * here were measured on Gaussian noise, whose rms is a third of its peak; a full-scale carrier
 * on the band edge (rms = peak, on the filter's poles) exceeds them: path 1 3.1e-6 of the
 * carrier, zoom 4's walk 1.8e-5 (its tiles, whose second FIR sums in float64, 8.2e-6; zoom 8's
 * tiles 6.6e-6, zoom 2's 6.1e-6), path 7 at zoom 2 7.4e-7.  The PC choices (zoom 8 below 16 frames per call,
 * zoom 4 below 32, zoom 2 below 512) within 6.5e-6, the head of zoom >= 16 (x8 + zoom 2's tiles or the
 * blocked passes) within 7.5e-6 -- the measured worst of the GPU tests + ~20 % (5.35e-6 and
 * 6.02e-6; the walk on the zf_n512_z8 fixture 6.07e-6; tests/test_gpu_pc.py PC_TOL / HEAD_TOL);
 * path 1: 2e-6.
 * 1 = blocked warm-up passes in the reference order (frames split over many waves),
 * 2 = blocked, fused commuted-order interior + exact edge windows, 3 = XA tiles (one wave per
 * frame and stage: all-pole cascade + 25-tap FIR + half-rate all-pole, lane states scanned;
 * each stage is one launch whose decimated output -- n_k/2 complex64 per frame -- is the next
 * stage's input in device memory), 4 = PC polyphase cascade (zoom 8: FIRs at falling
 * rates + the slow poles as zero-phase sections at rates 1/4 and 1/8, two launches, plus
 * rank-~10 frame-end maps; frames >= 16384 samples, <= 65535 frames per launch; zoom 4, 2
 * and the head of zoom >= 16 as below), 5 = the
 * same arithmetic as one launch with one workgroup per frame (the rate-1/4 intermediate
 * stays on chip); at zoom 4, path 5 is the two-stage
 * form of the walk (FIR, own-rate sections at rate 1/2, 41-tap FIR, 6 output-rate sections)
 * and path 4 its tiles (automatic below 32 frames per call); at zoom 2,
 * paths 4 / 5 run one-stage tiles in XA's factorisation (the
 * 4 sections forward at the input rate, a 25-tap FIR, their squares backward at half rate;
 * automatic below 512 frames per call); at zoom >= 16, paths 4 / 5 / 6 run PC / FC for the
 * first three stages and XA for the rest on its 1/8-rate output -- the automatic choice
 * wherever XA would take the batch (zoom 16 on cfg2's frames: 3.64 ms per 4096 frames with FC,
 * 5.01 with the walk, 6.35 with XA alone); 6 = FC, fast convolution (zoom 8, zoom 4 and the head
 * of zoom >= 16; elsewhere as 5): the model's impulse response truncated at |k| <= 768 (zoom 8)
 * / 512 (zoom 4) input samples (tail <= 1e-6 of its absolute sum) applied by overlap-save in
 * 8192-sample windows -- the residues' DFTs, the decimation folded into the spectrum with the
 * filter and the LO's modulation, one inverse DFT per window, one launch with one workgroup
 * per frame (or per run of windows below 1024 frames per call), the frame-end maps as for 5;
 * frames of >= 8192 samples below 2^31 bytes (cfg2's 4096 frames: 2.66 ms against the walk's
 * 4.18; cfg1's: 2.82 against the zoom-4 walk's 4.22); 7 = FC wherever a form exists, on request
 * only: as 6, plus zoom 2 (two residues of 4096 points, the one-stage model truncated at
 * |k| <= 256, 3840 outputs per window) and, at zoom >= 16, FC launches for the stages after the
 * head as well (three at a time, then two or one, while a launch's input has >= 16384 samples;
 * then as 6's tail) -- decimated IQ within 5.4e-7 of the reference's peak at zoom 2 and within
 * 6.9e-7 / 7.6e-7 at zoom 16 / 64 (measured worst 5.03e-7, 6.43e-7, 7.06e-7 + 7 %,
 * tests/test_gpu_fc2.py, profiles/r08fc2; 6's tails: 4e-6); cfg2's 4096 frames, ms per step,
 * automatic / 7: zoom 2 5.17 / 5.27 (FC wins between about 64 and 512 frames per call: 0.88
 * against 1.17 at 512), zoom 16 3.12 / 3.20, zoom 64 3.37 / 2.96; frames of >= 16384 samples
 * below 2^31 bytes, outside that as 6.  Path 3
 * needs every stage array below 2^31 bytes per frame; a forced path outside its domain
 * returns ZFFT_EUNSUPPORTED.  All produce the reference's rows within the fp32 parity gate
 * (zfft_plan.cpp auto_xa, use_fused, pc_fits, fc_fits). */
int zfft_plan_path(zfft_plan *plan, int32_t path);

/* Batched multi-IF (BASELINE config 4): one LO frequency per group of frames in a single
 * plan and launch chain.  Frame f of every zfft_process* / zfft_decimate call (f counted from
 * the call's first frame) is mixed with f_lo[(f / frames_per_lo) % n] instead of cfg.f_lo --
 * the reference's mixer (S:2090-2094) with f_demod per IF.  frames_per_lo = 1 interleaves
 * the IFs frame by frame; n = 0 restores cfg.f_lo; n = 1 replaces cfg.f_lo.  The LO table
 * holds n rows of n_samples complex64 (n <= 256, at most 4 GiB: ZFFT_ENOMEM beyond).  Zoom 1
 * never mixes (the reference skips zoomfft at ratio 1, S:2108): n > 1 is ZFFT_EINVAL there.
 * Waits for the plan's enqueued work. */
int zfft_plan_set_lo_frames(zfft_plan *plan, const double *f_lo, int32_t n, int32_t frames_per_lo);

/* Welch FFT schedule: 0 = automatic (one workgroup per frame for n_fft <= 16384, four-step
 * beyond), 1 = one workgroup per frame (n_fft <= 16384), 2 = four-step N1 x 256 (n_fft in
 * [4096, 65536]; its row pass forms only the bins the crop keeps when n_win <= n_fft / 8).
 * Same rows within the parity gate; diagnostics / A-B only.
 * Dynamic range (tests/test_gpu_welch_dynrange.py): under a full-scale component inside the band
 * every form's row amplitude 10^(row/40) is within 7.4e-7 of a full-scale bin (-123 dBc) of the
 * float64 reference, against 1.4e-7 for the same Welch in numpy float32.  The float32 row format
 * sets that figure: one unit in the last place of a row near -70 dB is 4.4e-7 of the bin's own
 * amplitude.  Away from the carrier's bin the worst are the four-step form with nperseg == n_fft,
 * 9.3e-8 at bins 0 and +-1 (it takes the mean off after the transform) and 7.2e-8 at bins
 * 255 mod 256 under a DC offset (its twiddles are products of table entries), and 1.9e-8 at
 * bin 0 from the float32 mean of the other forms. */
int zfft_plan_welch(zfft_plan *plan, int32_t mode);

/* Welch detector: how a frame's segments combine into its row.  With P_s[k] = |X_s,k|^2 /
 * (fs * sum(w^2)) the density of segment s (constant detrend, periodic window, 50 % overlap,
 * fs the original rate; one-sided rows: the doubled bins, per segment),
 *   ZFFT_AVG_MEAN    mean_s P_s[k] -- scipy.signal.welch's default and the reference's call;
 *                    the plan's default, the same kernels and rows as without this call;
 *   ZFFT_AVG_MEDIAN  median_s P_s[k] / bias(nseg) -- scipy.signal.welch(average='median'):
 *                    numpy's median (even nseg: the mean of the two middle values), bias(n) =
 *                    1 + sum_{i=1..(n-1)/2} (1/(2i+1) - 1/(2i)), computed in double on the host.
 *                    An impulse that sits in a few segments leaves the row where it was;
 *   ZFFT_AVG_MAX     max_s P_s[k], no bias: the peak (max-hold) detector over the frame, for
 *                    transmissions shorter than it (the mean dilutes them by nseg).
 * Rows stay 20*log10 of the fftshift-cropped bins, zfft_plan_row_length long; a zero bin gives
 * -inf, a NaN in any segment NaN.  A frame with one segment (nseg 1, e.g. the short-input
 * branch L_d < n_fft) gives the same row in all three (bias(1) = 1).  Valid wherever mean is:
 * every n_fft, both zfft_plan_welch forms, any number of frames and segments.  The mode holds
 * for every later zfft_process* / zfft_ring_process call until it is changed; any other value
 * is ZFFT_EINVAL.  Median and max keep every segment's bins in a device scratch (nseg * n_win
 * floats per frame; the frames of a call go in chunks of at most 1 GiB of it, one frame at
 * least) and reduce them with a second kernel: with zfft_plan_timing they report
 * "welch_segs" / "welch4_segs" then "welch_select" per chunk in place of "welch_rows" /
 * "welch4". */
enum zfft_average { ZFFT_AVG_MEAN = 0, ZFFT_AVG_MEDIAN = 1, ZFFT_AVG_MAX = 2 };
int zfft_plan_average(zfft_plan *plan, int32_t mode);

/* Time-resolved waterfall: segments per waterfall line.  0 (default) = the whole frame: one row
 * per frame, exactly the kernels and bytes of a plan that never called this.  g >= 1: a frame's
 * nseg segments, in the order Welch receives them (after flip_input), form R = ceil(nseg / g)
 * groups of g consecutive segments (the last group holds the remaining 1..g); row r is the
 * plan's detector over group r:
 *   mean   20 log10( (1/n_r) sum_{s in group r} P_s[k] )
 *   median 20 log10( median_{s in group r} P_s[k] / bias(n_r) )   (numpy's median, scipy's bias)
 *   max    20 log10( max_{s in group r} P_s[k] )
 * with P_s and the crop as in zfft_plan_average, n_r the group's size: g = 1 is
 * scipy.signal.spectrogram(mode='psd') through the reference's crop and dB.  g >= nseg gives
 * R = 1 and takes the g = 0 path.  Rows of frame f are rows_out[(f R + r) n_win ...], in time
 * order, so zfft_process* needs n_frames * R * n_win floats; R = zfft_line_count(...).  g < 0 is
 * ZFFT_EINVAL.  Which kernels form the lines is the plan's choice and no part of this interface
 * (zfft_plan_timing_names tells what ran). */
int zfft_plan_segments_per_line(zfft_plan *plan, int32_t g);
/* No plan, no GPU (like zfft_decimated_length): rows per frame of n_samples input samples;
 * 1 for g = 0, for the short-input branch (L_d < n_fft) and whenever g >= nseg.  -1 for
 * n_samples < 1, n_fft < 2, a zoom that is no power of two, or g < 0. */
int64_t zfft_line_count(int64_t n_samples, int32_t zoom, int32_t n_fft, int32_t g);
/* Centre time of every line in seconds from the frame's first sample, at the input rate fs: the
 * mean over the group of scipy.signal.spectrogram's t_s = (s step + nperseg/2) zoom / fs.
 * *count = zfft_line_count(...); ZFFT_EINVAL (with *count set) when max is smaller. */
int zfft_line_times(int64_t n_samples, int32_t zoom, int32_t n_fft, double fs, int32_t g,
                    double *t_out, int32_t max, int32_t *count);
/* zfft_ring_process for a plan with g >= 1 (any plan: g = 0 gives one line): up to max_lines rows
 * of the drained frame, *produced of them (0: the frame was shorter than n_fft).  ZFFT_EINVAL
 * before anything is taken when max_lines < zfft_line_count(ring capacity, ...).  Plain
 * zfft_ring_process on a plan with g >= 1 is ZFFT_EINVAL, before a frame is taken. */
int zfft_ring_process_lines(zfft_ring *ring, zfft_plan *plan, float *rows_out, int32_t max_lines,
                            int32_t *produced);

/* Persistence (digital-phosphor) spectrum: for every column of the plan's rows a histogram of
 * the levels seen, accumulated on the device from rows the caller pushes -- the model is the
 * waterfall ring: nothing is hidden inside zfft_process*, and a plan that never enables it
 * allocates and launches nothing for it.
 * Binning rule (float32 throughout, reproducible bit for bit in numpy float32):
 *   lo  = (float)db_min
 *   inv = (float)(levels / (db_max - db_min))     the division in double, rounded once
 *   t   = (v - lo) * inv                          each operation rounded to float32, no
 *                                                 contraction into a fused multiply-add
 * and v is counted in cell (int)t of its column when t >= 0 and t < levels; any other value is
 * counted nowhere: NaN, +-inf, the -inf of a zero bin, levels outside the range, db_max itself.
 * Level 0 is the lowest; the table is hist[level * n_win + j], column j as in a row; columns at
 * or beyond zfft_plan_row_length stay 0.  rows_seen grows by `count` with every push, whatever
 * its values.  Counts are uint32 and wrap modulo 2^32 when a cell sees more than 2^32 - 1
 * values between decays or resets: zfft_persistence_decay is the remedy.
 * Every zfft_persistence_* call on a plan with persistence off returns ZFFT_EINVAL
 * (zfft_persistence_shape after reporting 0 levels).  With zfft_plan_timing on, a push reports
 * its kernel as "persist_hist" (zfft_plan_timings then describes the push, the last timed call). */
/* levels = 0 (default): off, frees the table.  levels in [2, 256], db_min < db_max finite:
 * allocates and zeroes a table of levels x n_win uint32 counts (level-major, column j as in a
 * row) and a row counter.  Anything else ZFFT_EINVAL.  Re-enabling with new parameters resets. */
int zfft_plan_persistence(zfft_plan *plan, int32_t levels, double db_min, double db_max);
int zfft_persistence_shape(const zfft_plan *plan, int32_t *levels, int32_t *cols);
/* Bin `count` rows of n_win floats (row stride n_win; only the first zfft_plan_row_length
 * columns of each row are read).  Enqueued on hip_stream, no sync; ordered after earlier
 * work on that stream (as zfft_waterfall_push_device). */
int zfft_persistence_push_device(zfft_plan *plan, const float *d_rows, int32_t count, void *hip_stream);
int zfft_persistence_push(zfft_plan *plan, const float *rows /* host */, int32_t count);  /* synchronous */
/* every count c -> floor(c * keep) and rows_seen likewise, in double; 0 <= keep <= 1 */
int zfft_persistence_decay(zfft_plan *plan, double keep);
int zfft_persistence_reset(zfft_plan *plan);
/* waits for the plan's enqueued pushes; hist_out levels*n_win uint32; rows_seen may be NULL */
int zfft_persistence_read(zfft_plan *plan, uint32_t *hist_out, uint64_t *rows_seen);

/* Signal detection on rows: per row a noise floor, the emissions above floor + threshold, and
 * per column a count of how often it was part of one -- from rows the caller holds on the
 * device, in the model of the ring and of persistence: nothing is hidden inside zfft_process*,
 * and a plan that never enables it allocates and launches nothing for it.
 * A row is the first n = zfft_plan_row_length(plan) floats of a stride of n_win.  Every value
 * here is in row units, and rows are 20*log10(PSD): a POWER ratio of 4 is 12.04 units, not
 * 6.02 -- threshold_db is a difference of row values, nothing else.
 * The rule (float32 values, reproducible bit for bit in numpy float32):
 *   1. population: the finite values of the row; NaN, +inf and -inf are left out.  m = their
 *      number.  m == 0: floor = NaN and the row has no emissions.
 *   2. floor: the value of 0-based rank k = (int64)floor(q * (double)(m - 1)) among the finite
 *      values in ascending order, q the plan's quantile in [0, 1] (q = 0.5: the lower median).
 *      No interpolation: the floor is one of the row's own values, bit for bit (-0.0 and 0.0
 *      compare equal; which of the two a zero floor is, is not defined).  numpy:
 *      np.sort(finite)[k].
 *   3. thr = floor + (float)threshold_db, one float32 addition; threshold_db any finite double.
 *      Column j is on when v[j] >= thr: +inf is on, NaN and -inf are off.
 *   4. an emission is a maximal run [first, last] of consecutive on columns with
 *      last - first + 1 >= min_width (min_width >= 1).  Gaps are not bridged.
 *   5. its record: first, last, peak = the lowest column of the run that holds the run's
 *      maximum, peak_db = that value, unchanged.
 *   6. per row i: floor[i]; found[i] = the number of kept runs, those beyond the cap included;
 *      events[i * K + 0 .. K - 1] = the first min(found, K) runs in ascending column order, the
 *      remaining slots all-zero records (K = max_per_row in [1, 32]): the outputs are fully
 *      defined and need no clearing by the caller.
 *   7. occupancy: occ[j], a uint32 per column (n_win in all), grows by 1 for every column of
 *      every kept run, recorded within K or not; columns at or beyond n stay 0.  rows_seen grows
 *      by `count` with every call.  Counts wrap modulo 2^32.
 * Every zfft_detect* call on a plan with detection off returns ZFFT_EINVAL (zfft_detect_shape
 * after reporting max_per_row 0).  With zfft_plan_timing on, a call reports its kernel as
 * "detect_rows" (zfft_plan_timings then describes that call, the last timed one). */
typedef struct zfft_emission {
  int32_t first, last, peak;
  float peak_db;
} zfft_emission; /* 16 bytes */
/* max_per_row = 0 (default): off, frees the occupancy table.  Otherwise max_per_row in [1, 32],
 * quantile in [0, 1], threshold_db finite, min_width in [1, n_win]; anything else ZFFT_EINVAL.
 * Re-enabling resets the occupancy. */
int zfft_plan_detect(zfft_plan *plan, double quantile, double threshold_db, int32_t min_width, int32_t max_per_row);
int zfft_detect_shape(const zfft_plan *plan, int32_t *max_per_row, int32_t *cols);
/* count rows of stride n_win on the device; outputs on the device: count floats, count int32,
 * count * max_per_row records (16-byte aligned).  Enqueued on hip_stream, no sync; ordered after
 * earlier work on that stream (as zfft_persistence_push_device). */
int zfft_detect_device(zfft_plan *plan, const float *d_rows, int32_t count, float *d_floor, int32_t *d_found,
                       zfft_emission *d_events, void *hip_stream);
/* host rows and host outputs, synchronous */
int zfft_detect(zfft_plan *plan, const float *rows, int32_t count, float *floor_out, int32_t *found_out,
                zfft_emission *events_out);
/* waits for the plan's enqueued calls; occ_out n_win uint32; rows_seen may be NULL */
int zfft_detect_occupancy(zfft_plan *plan, uint32_t *occ_out, uint64_t *rows_seen);
int zfft_detect_reset(zfft_plan *plan); /* zeroes occupancy and rows_seen */

/* A local noise floor per column (order-statistic CFAR).  The row-global floor is right only
 * where the floor is flat; under a decimator's roll-off, a shaped passband or beside a strong
 * wideband emission the quiet part of a row loses its weak emissions and the loud part turns
 * into one emission.  zfft_plan_detect_local(plan, half_window, guard) judges every column
 * against an order statistic of the columns around it instead:
 *   half_window = 0 (then guard must be 0; the default): the row-global floor, everything above.
 *   Otherwise 1 <= half_window <= 128 and 0 <= guard <= 128.  With h = half_window, gd = guard,
 *   n = zfft_plan_row_length(plan) and q, threshold_db, min_width, K those of zfft_plan_detect:
 *   1. reference cells of column j (0 <= j < n): the columns c with gd < |c - j| <= gd + h and
 *      0 <= c < n.  The window is cut at the row's ends: it neither wraps nor mirrors, so a
 *      column near an end has fewer cells, all on one side at the very end.  Column j and its gd
 *      neighbours on either side are never reference cells.
 *   2. population: the finite values among the reference cells, m_j of them; NaN, +inf and -inf
 *      are left out, as in the global rule.
 *   3. floor_j: the value of 0-based rank (int64)floor(q * (double)(m_j - 1)) among them in
 *      ascending order -- one of the row's own values, bit for bit (which of -0.0 and 0.0 a zero
 *      floor is, is not defined).  m_j == 0: floor_j = NaN.  numpy: np.sort(w[np.isfinite(w)])[k].
 *   4. thr_j = floor_j + (float)threshold_db, one float32 addition; column j is on when
 *      v[j] >= thr_j: +inf is on, NaN and -inf are off, every column with floor_j = NaN is off.
 *   5. rules 4-7 of zfft_plan_detect hold unchanged: the runs, the records, found, the zeroed
 *      slots and the occupancy.
 *   6. floor[i] of zfft_detect* stays the row-global floor (rule 2 of zfft_plan_detect), the
 *      row's one-number summary.
 * ZFFT_EINVAL while detection is off and for arguments outside these ranges.  A call zeroes the
 * occupancy and rows_seen (counts made under two rules do not add).  zfft_plan_detect(...,
 * max_per_row = 0) puts the mode back to global; a zfft_plan_detect call on a plan that is on
 * keeps it.  zfft_detect_device and zfft_detect follow the plan's mode; the floors of a pass go
 * through a device scratch of the plan's, at most 256 MiB (larger calls run in passes), freed
 * when detection is switched off and never allocated in global mode.  With zfft_plan_timing on a
 * local-mode call reports "detect_floor" then "detect_rows", once per pass. */
int zfft_plan_detect_local(zfft_plan *plan, int32_t half_window, int32_t guard);
int zfft_detect_local_shape(const zfft_plan *plan, int32_t *half_window, int32_t *guard); /* 0, 0: global */
/* floor_j of rule 3 for `count` rows, as float rows of stride n_win (an SNR, a floor trace on
 * the display).  A pure function of the rows: no occupancy, no rows_seen.  ZFFT_EINVAL in global
 * mode.  Device form: columns at or beyond n are left untouched; enqueued on hip_stream, no sync,
 * ordered after earlier work on that stream; reports "detect_floor".  Host form: those columns
 * are written as NaN; synchronous. */
int zfft_detect_floors_device(zfft_plan *plan, const float *d_rows, int32_t count, float *d_floors, void *hip_stream);
int zfft_detect_floors(zfft_plan *plan, const float *rows, int32_t count, float *floors_out);

/* Emission tracks: the detector's runs linked across rows on the device, so that a carrier that
 * stays, a burst, a chirp are one record each -- when it began and ended, the band it covered,
 * where and how strong its peak was -- instead of one record per row.  In the model of the
 * detector it belongs to: nothing runs inside zfft_process*, the caller hands over the very
 * buffers zfft_detect_device wrote, and a plan that never enables it allocates and launches
 * nothing for it.  The rule (integers throughout, reproducible bit for bit in numpy;
 * tests/track_ref.py):
 *   Rows given to the tracker are numbered t = 0, 1, 2, ... from the last reset (64-bit; the
 *   kernels hold row * 32 + slot in 64 bits, so t < 2^58).
 *   1. nodes: row t contributes its recorded runs, the slots s = 0 .. min(max(found, 0), K) - 1
 *      of the detector's output for that row, K the plan's max_per_row; each a record (first,
 *      last, peak, peak_db) as rules 4-6 of zfft_plan_detect define it.  A row with found > K
 *      counts once in truncated_rows; its runs beyond K do not exist for the tracker.
 *   2. links: runs a (row t_a) and b (row t_b) with 1 <= t_b - t_a <= gap + 1 are linked when
 *      first_a <= last_b + slack && first_b <= last_a + slack.  gap in [0, 7]: the rows an
 *      emission may be absent for (keying, fading); slack in [0, 64]: 0 means the two runs share
 *      a column, 1 that they may merely touch.  The rows in between do not matter; runs of one
 *      row are never linked to each other.
 *   3. a track is a connected component of that graph.  Its record, zfft_track: row_first,
 *      row_last the lowest and highest row of its runs; cells the sum of last - first + 1 and
 *      runs the number of its runs; col_first = min first, col_last = max last; slot_first the
 *      lowest slot among its runs in row_first; peak_db the maximum of its runs' peak_db as a
 *      float comparison (-0.0 and 0.0 are equal; a zero maximum is reported as 0.0);
 *      (peak_row, peak_col) the lexicographically lowest (row, peak) among the runs that hold
 *      that maximum; reserved = 0.  (row_first, slot_first) names a track uniquely.
 *   4. closing: after S rows have been given a track is closed when row_last + gap + 1 < S -- no
 *      later row can reach it -- and open otherwise.  A closed track with row_last - row_first
 *      + 1 >= min_rows (min_rows >= 1) is reported; any other closed track counts in
 *      short_tracks and is forgotten.
 *   5. order: zfft_track_read returns the reported tracks not yet read in ascending (row_last,
 *      row_first, slot_first) and removes them from the store.  The closed set after S rows is
 *      {row_last <= S - gap - 2}, so the sequence over all reads is the same however the rows
 *      were cut into calls and however the reads were interleaved with them.
 *   6. store: at most max_tracks (1 .. 2^22) reported tracks wait unread; one that finds the
 *      store full counts in dropped and is lost (which ones are lost is not defined).  With
 *      dropped == 0 every output is exactly this rule.
 *   7. flush: zfft_track_flush closes every open track as it stands, reporting or counting it by
 *      min_rows, in the order of rule 5 among themselves.  The row counter does not advance;
 *      later rows link to nothing earlier.
 *   8. open tracks: zfft_track_open copies the open tracks as they stand now, in ascending
 *      (row_first, slot_first), and changes nothing.  There are at most (gap + 1) * K of them;
 *      an endless carrier never closes, and this call is how a display sees it.
 *   9. input: records as the detector writes them -- ascending, disjoint, 0 <= first <= peak <=
 *      last, peak_db not NaN.  The host form checks the slots it will use and returns
 *      ZFFT_EINVAL otherwise; in the device form other contents give undefined track values.
 *      Columns are only ever compared, never used as addresses: the kernels stay in bounds
 *      whatever the records hold.  found < 0 is 0 and found > K is K, as in rule 1.
 * Tracking belongs to the detector and needs detection on (K is the detector's):
 * zfft_plan_detect(..., max_per_row = 0) switches it off and frees it, and a zfft_plan_detect call
 * that changes max_per_row while tracking is on resets the tracker.  Every zfft_track_* call on a
 * plan with tracking off returns ZFFT_EINVAL (zfft_track_shape after reporting max_tracks 0).
 * zfft_track_push_device is enqueued on its stream with no sync, ordered after earlier work on
 * that stream and after the plan's earlier calls on any stream; read, open, state and flush wait
 * for what is enqueued.  With zfft_plan_timing on a push reports its launches by name
 * ("track_label", "track_seam", ...: zfft_plan_timings then describes that push). */
typedef struct zfft_track {
  int64_t row_first, row_last; /* lowest and highest row of its runs */
  int64_t peak_row;
  uint64_t cells; /* sum of last - first + 1 over its runs */
  uint64_t runs;  /* number of runs */
  int32_t col_first, col_last; /* min first, max last */
  int32_t peak_col;
  int32_t slot_first; /* lowest slot among its runs in row_first */
  float peak_db;      /* max peak_db, as a float comparison */
  int32_t reserved;   /* 0 */
} zfft_track; /* 64 bytes */
typedef struct zfft_track_stats {
  uint64_t rows_seen, open, unread, dropped, short_tracks, truncated_rows;
} zfft_track_stats;
/* max_tracks = 0: off, frees everything.  Otherwise gap in [0, 7], slack in [0, 64], min_rows >= 1,
 * max_tracks in [1, 2^22]; anything else, or detection off, ZFFT_EINVAL.  A call resets the tracker. */
int zfft_plan_track(zfft_plan *plan, int32_t gap, int32_t slack, int32_t min_rows, int32_t max_tracks);
int zfft_track_shape(const zfft_plan *plan, int32_t *gap, int32_t *slack, int32_t *min_rows, int32_t *max_tracks);
/* count rows' found (count int32) and records (count * max_per_row) on the device, 1 <= count <= 2^26;
 * `stream` is a hipStream_t like every hip_stream of this header (its ordering case, behind a
 * stalled stream, is in tests/test_gpu_track.py) */
int zfft_track_push_device(zfft_plan *plan, const int32_t *d_found, const zfft_emission *d_events, int32_t count,
                           void *stream);
/* host found and records, checked by rule 9; synchronous */
int zfft_track_push(zfft_plan *plan, const int32_t *found, const zfft_emission *events, int32_t count);
/* at most `max` reported tracks into out, *n their number; removes them from the store */
int zfft_track_read(zfft_plan *plan, zfft_track *out, int32_t max, int32_t *n);
/* at most `max` open tracks into out, *n their number; changes nothing */
int zfft_track_open(zfft_plan *plan, zfft_track *out, int32_t max, int32_t *n);
int zfft_track_flush(zfft_plan *plan);
int zfft_track_state(zfft_plan *plan, zfft_track_stats *out);
int zfft_track_reset(zfft_plan *plan); /* everything back to zero, the store emptied */

/* Display viewport: a second, display-sized image kept on the device, reduced from the rows the
 * caller pushes as a spectrum analyser's display detector does -- every pixel the max, min or
 * mean of all the columns and rows that fall into it -- in the model of the ring, persistence
 * and the detector: nothing is hidden inside zfft_process*, and a plan that never enables it
 * allocates and launches nothing for it.  The reference-compatible ring (zfft_waterfall_*) is
 * untouched by all of this.
 * A row is the first n = zfft_plan_row_length(plan) floats of a stride of n_win.  The rule
 * (MAX and MIN reproducible bit for bit in numpy float32):
 *   1. geometry: 0 <= col0 < col1 <= n, span = col1 - col0, 1 <= width <= span (a pixel never
 *      covers less than one column: no upsampling), 1 <= height <= 8192, height * width <= 2^25,
 *      1 <= rows_per_line <= 65536, detector one of zfft_view_detector.  Pixel x covers the
 *      columns [e(x), e(x + 1)), e(x) = col0 + floor(x * span / width) in int64
 *      (zfft_viewport_edge): bucket sizes differ by at most one.
 *   2. groups: pushed rows are counted from the enable or the last zfft_viewport_reset, across
 *      pushes; rows [L m, (L + 1) m), m = rows_per_line, form line L.  A group a push leaves
 *      incomplete stays pending on the device (`pending` = its rows so far) and a later push
 *      completes it: any split of the same rows into pushes gives the same lines, bit for bit
 *      for MAX and MIN, within the row gate (1e-3 dB) for MEAN.
 *   3. cell value over the set S of m rows x the bucket's columns:
 *        ZFFT_VIEW_MAX   np.fmax.reduce(S): NaN is ignored, an all-NaN S gives NaN, +-inf take
 *                        part; whether a zero result is -0.0 or 0.0 is not defined;
 *        ZFFT_VIEW_MIN   np.fmin.reduce(S), likewise;
 *        ZFFT_VIEW_MEAN  20 log10(sum_S 10^(v/20) / |S|): rows are 20 log10(PSD), so this is the
 *                        mean PSD.  Any NaN in S gives NaN, -inf contributes 0, +inf gives +inf,
 *                        an all-zero sum -inf.  10^(v/20) is float32, the sums are float64 (the
 *                        pending group's too), in any order.
 *   4. image: completed lines go into a ring of `height` lines in the waterfall ring's
 *      convention, img[i] == ring[(i + off) mod height] and off += scroll per line: with scroll
 *      +1 the newest line is image row height - 1 and the lines above it are older one by one,
 *      with -1 it is row 0 and the lines below are older (the waterfall ring's scroll +1 keeps
 *      the reference's roll, newest at row H - 2; the viewport does not).  The direction is cfg.scroll as
 *      it is at the enable or the reset (zfft_waterfall_reset changes cfg.scroll).  Lines not yet
 *      written are NaN; no grid, no tick stamps.  When one push completes more than `height`
 *      lines the last `height` remain; `lines` and the hold traces count all of them.
 *   5. traces, `width` floats each: last = the newest completed line; max_hold / min_hold = the
 *      per-pixel fmax / fmin of every line completed since the enable, the reset or
 *      zfft_viewport_hold_reset.  All NaN before the first line.
 *   6. render: zfft_waterfall_render's pixel formula with the plan's colormap and levels
 *      (zfft_waterfall_colormap / _levels need no ring: a plan too narrow for the ring, n_win
 *      < 40, can have a viewport); NaN has alpha 0.
 * Every zfft_viewport_* call on a plan with the viewport off returns ZFFT_EINVAL
 * (zfft_viewport_shape after reporting 0 x 0).  With zfft_plan_timing on, a push reports its
 * kernels as "view_lines", then "view_finish" when a second launch merged the pending group,
 * a split group's slices or the workgroups' hold partials. */
enum zfft_view_detector { ZFFT_VIEW_MAX = 0, ZFFT_VIEW_MIN = 1, ZFFT_VIEW_MEAN = 2 };
/* height = 0 (default): off, frees everything.  Valid arguments (rule 1) allocate the ring, the
 * traces and the pending accumulator, all NaN / empty; anything else ZFFT_EINVAL.  Re-enabling
 * with any parameters resets the viewport: rows are not kept, so older lines cannot be reduced
 * again to a new geometry (the row history below keeps them: zfft_history_replay_viewport). */
int zfft_plan_viewport(zfft_plan *plan, int32_t height, int32_t width, int32_t col0, int32_t col1,
                       int32_t detector, int32_t rows_per_line);
/* No plan, no GPU: e(x) of rule 1 for 0 <= x <= width; -1 for invalid arguments. */
int64_t zfft_viewport_edge(int32_t col0, int32_t col1, int32_t width, int32_t x);
int zfft_viewport_shape(const zfft_plan *plan, int32_t *height, int32_t *width);
/* count rows of stride n_win on the device; only columns [col0, col1) are read.  Enqueued on
 * hip_stream, no sync; ordered after earlier work on that stream (as zfft_persistence_push_device). */
int zfft_viewport_push_device(zfft_plan *plan, const float *d_rows, int32_t count, void *hip_stream);
int zfft_viewport_push(zfft_plan *plan, const float *rows /* host */, int32_t count);  /* synchronous */
/* rows pushed, lines completed and the pending group's rows since the enable / reset; any NULL */
int zfft_viewport_state(zfft_plan *plan, uint64_t *rows_seen, uint64_t *lines, int32_t *pending);
/* these wait for the plan's enqueued pushes.  img_out height*width floats in image order;
 * last / max_hold / min_hold width floats each, NULL = skip */
int zfft_viewport_read(zfft_plan *plan, float *img_out);
int zfft_viewport_traces(zfft_plan *plan, float *last, float *max_hold, float *min_hold);
int zfft_viewport_hold_reset(zfft_plan *plan); /* max_hold and min_hold back to NaN, nothing else */
/* image, traces, pending group and counters as after the enable; re-reads cfg.scroll */
int zfft_viewport_reset(zfft_plan *plan);
/* RGBA8, height*width*4 bytes: into device memory on hip_stream (no sync), or to the host */
int zfft_viewport_render_device(zfft_plan *plan, uint8_t *d_rgba, void *hip_stream);
int zfft_viewport_render(zfft_plan *plan, uint8_t *rgba_out);
/* The per-line display in one round trip (as zfft_waterfall_push_render): count >= 0 host rows
 * staged in page-locked memory and pushed, the image rendered and copied, one wait.  An image of
 * at most 4 MiB is written straight into a page-locked rgba_out (zfft_host_alloc). */
int zfft_viewport_push_render(zfft_plan *plan, const float *rows, int32_t count, uint8_t *rgba_out);

/* Row history: the rows the caller pushes kept on the device in a ring of capacity_rows rows, as
 * float32 or quantised to 16- or 8-bit codes on a fixed level scale, so that what has scrolled
 * past can be reduced again -- to another window of columns, another rows_per_line, another
 * detector, an older stretch of time -- which the viewport alone cannot do.  In the model of the
 * ring, persistence, the detector and the viewport: nothing is hidden inside zfft_process*, and
 * a plan that never enables it allocates and launches nothing for it.
 * A row is the first n = zfft_plan_row_length(plan) floats of a stride of n_win; the store holds
 * those n columns (capacity_rows x n x {4, 2, 1} bytes, each row padded to a multiple of 16
 * elements).  The rule:
 *   1. rows are numbered from 0 since the enable or the last zfft_history_reset, across pushes;
 *      rows_seen grows by `count` with every push.  The store keeps the last min(rows_seen,
 *      capacity) rows, oldest = rows_seen - that; a push of more than capacity rows keeps its
 *      last capacity.
 *   2. quantiser (float32 throughout, reproducible bit for bit in numpy float32; K = 254 for U8,
 *      65534 for U16): lo = (float)db_min, inv = (float)(K / (db_max - db_min)), step =
 *      (float)((db_max - db_min) / K), both divisions in double and rounded once.
 *        pack    NaN -> code 0; otherwise t = (v - lo) * inv (a float32 difference, then a
 *                float32 product) and code = 1 + (int)rintf(fminf(fmaxf(t, 0), K)), ties to even:
 *                -inf and every level at or below db_min give code 1, +inf and every level at or
 *                above db_max give code K + 1.
 *        unpack  code 0 -> NaN; otherwise lo + (float)(code - 1) * step, a float32 product, then
 *                a float32 sum, never a fused multiply-add.
 *      The code does not decrease with v and the value does not decrease with the code, pack(
 *      unpack(c)) == c for every code, and inside [db_min, db_max] the round trip is off by at
 *      most 0.513 step.  ZFFT_HISTORY_F32 stores and returns the value unchanged (a NaN comes
 *      back as a NaN) and ignores the two levels.  zfft_history_codes / _values are the quantiser
 *      itself, on the host.
 *   3. read: the unpacked rows [first, first + count) as float rows of stride n_win, valid input
 *      to zfft_viewport_push_device, zfft_persistence_push_device and zfft_detect_device on the
 *      same stream.  ZFFT_EINVAL unless oldest <= first and first + count <= rows_seen.  Columns
 *      at or beyond n are left untouched on the device and written as NaN on the host path.
 *   4. view: rule 1 and rule 3 of zfft_plan_viewport applied to the unpacked rows v', with no
 *      state: the window's geometry limits are the viewport's (0 <= col0 < col1 <= n, 1 <= width
 *      <= col1 - col0, 1 <= lines <= 8192, lines * width <= 2^25, 1 <= rows_per_line <= 65536,
 *      a zfft_view_detector); pixel x covers the columns [e(x), e(x + 1)) of zfft_viewport_edge;
 *      line L is img[L * width + x], in time order, L = 0 the oldest, over the rows [first + L m,
 *      first + (L + 1) m), m = rows_per_line.  `first` is signed and may lie before `oldest` or
 *      run past rows_seen: a line with any row not in the store is all NaN (an incomplete group
 *      is never shown, as in the viewport).  MAX and MIN are the same bits whatever form ran;
 *      MEAN = 20 log10(sum 10^(v'/20) / |S|) with 10^x in float32 and the sums in float64.  To
 *      get the lines a live viewport produced, choose `first` congruent to the row at which that
 *      viewport was last reset, modulo m.
 *   5. render: the view through zfft_waterfall_render's pixel formula with the plan's colormap
 *      and levels, NaN with alpha 0, lines x width x 4 bytes: the bytes zfft_viewport_render
 *      gives for a viewport that holds the same lines.
 *   6. replay: zfft_history_replay_viewport(plan, first) needs both features on.  It is
 *      zfft_viewport_reset followed by the stored rows [max(first, oldest), rows_seen) unpacked
 *      and pushed in order (through a plan-owned float scratch, in chunks of at most 64 MiB, on
 *      the plan's stream, one wait at the end): after zfft_plan_viewport with a new geometry it
 *      rebuilds image, pending group and hold traces, and live pushes carry on from there.
 * Every zfft_history_* call on a plan with the store off returns ZFFT_EINVAL (zfft_history_shape
 * after reporting capacity 0).  With zfft_plan_timing on, a push reports its kernel as
 * "history_pack", a read as "history_unpack" and a view as "history_view", then "history_finish"
 * when a second launch combined the slices of long groups. */
enum zfft_history_format { ZFFT_HISTORY_F32 = 0, ZFFT_HISTORY_U16 = 1, ZFFT_HISTORY_U8 = 2 };
typedef struct zfft_history_window {
  int64_t first;
  int32_t rows_per_line, lines, col0, col1, width, detector;
} zfft_history_window;
/* capacity_rows = 0 (default): off, frees the store.  Otherwise capacity_rows >= 1, format one of
 * zfft_history_format and, for U16 / U8, db_min < db_max finite; anything else ZFFT_EINVAL.  An
 * allocation the device refuses is ZFFT_ENOMEM and leaves the store off.  Re-enabling resets. */
int zfft_plan_history(zfft_plan *plan, int64_t capacity_rows, int32_t format, double db_min, double db_max);
int zfft_history_shape(const zfft_plan *plan, int64_t *capacity, int32_t *cols, int32_t *format);
/* count rows of stride n_win on the device; only the first n columns are read.  Enqueued on
 * hip_stream, no sync; ordered after earlier work on that stream (as zfft_viewport_push_device). */
int zfft_history_push_device(zfft_plan *plan, const float *d_rows, int32_t count, void *hip_stream);
int zfft_history_push(zfft_plan *plan, const float *rows /* host */, int32_t count);  /* synchronous */
int zfft_history_state(zfft_plan *plan, uint64_t *rows_seen, uint64_t *oldest); /* either may be NULL */
int zfft_history_read_device(zfft_plan *plan, int64_t first, int32_t count, float *d_rows, void *hip_stream);
int zfft_history_read(zfft_plan *plan, int64_t first, int32_t count, float *rows_out); /* host, synchronous */
/* w->lines * w->width floats: into device memory on hip_stream (no sync), or to the host */
int zfft_history_view_device(zfft_plan *plan, const zfft_history_window *w, float *d_img, void *hip_stream);
int zfft_history_view(zfft_plan *plan, const zfft_history_window *w, float *img_out);      /* synchronous */
int zfft_history_render(zfft_plan *plan, const zfft_history_window *w, uint8_t *rgba_out); /* synchronous */
int zfft_history_replay_viewport(zfft_plan *plan, int64_t first);                          /* synchronous */
int zfft_history_reset(zfft_plan *plan); /* rows_seen and oldest back to 0 */
/* No plan, no GPU (like zfft_viewport_edge): rule 2 on n values; format U16 or U8, codes as
 * uint16 in both.  ZFFT_EINVAL for F32, bad levels or a code above K + 1. */
int zfft_history_codes(int32_t format, double db_min, double db_max, const float *v, int64_t n, uint16_t *codes_out);
int zfft_history_values(int32_t format, double db_min, double db_max, const uint16_t *codes, int64_t n, float *v_out);

/* Channel taps: narrowband complex streams out of the wideband input.  A tap is a digital
 * down-converter with state -- an oscillator, a real FIR low-pass, an integer decimation -- on the
 * samples the plan is given, not on its rows; a plan holds up to max_taps of them, and one push of
 * a contiguous stretch of input makes every open tap emit the output samples that fall in it.  The
 * state between pushes stays on the device.  Off by default: a plan that never calls
 * zfft_plan_taps allocates and launches nothing.  The rule (reference: tests/tap_ref.py):
 *   1. samples: the plan counts input samples n = 0, 1, ... from zfft_plan_taps, or from
 *      zfft_tap_reset(plan, n0), which restarts the count at n0 (0 <= n0 <= 2^62), zeroes the
 *      carry and leaves the open taps open as if opened at n0.  x[n] is the input as the plan's
 *      in_dtype loader defines it in float32 (all four in_dtype values), and x[n] = 0 for the
 *      samples before the start.  flip_input = 1 has no continuous time axis: zfft_plan_taps
 *      returns ZFFT_EUNSUPPORTED.
 *   2. a tap has freq_word fw, an integer in [-2^31, 2^31): its centre frequency is fw / 2^32
 *      cycles per input sample; decim D in [1, 512]; n_taps T in [1, max_len] (max_len <= 2048)
 *      real float32 taps h[0 .. T); n_open, the count at which it was opened.
 *   3. outputs: y[m] = sum_{k < T} h[k] x[m D - k] exp(-2 pi i ((fw (m D - k)) mod 2^32) / 2^32)
 *      for every m with m D >= n_open.  The phase is integer arithmetic on the plan-wide count:
 *      taps opened at different times are phase-coherent with each other, and nothing drifts or
 *      loses precision with time (the phase wraps exactly; the count is 64-bit).
 *   4. a push of n_samples at count n0 emits, per tap, the m with max(n0, n_open) <= m D <
 *      n0 + n_samples: ceil((n0 + n_samples) / D) - ceil(max(n0, n_open) / D) samples
 *      (zfft_tap_counts, for the next push).  The push writes complex64 outputs into one buffer,
 *      the open taps in slot order back to back.  The outputs do not depend on how the stream is
 *      cut into pushes, bit for bit.
 *   5. a newly opened tap sees the true past: the plan carries the last max_len - 1 input samples
 *      as complex64 whether or not any tap is open.
 *   6. the group delay (T - 1) / 2 input samples is reported (zfft_tap_info), not compensated.
 *   7. arithmetic, the form the FC decimator uses for its LO: c[k] = float32(h[k] exp(+2 pi i
 *      ((fw k) mod 2^32) / 2^32)), built on the host in float64 (zfft_tap_table); y[m] = rot(m)
 *      sum_k c[k] x[m D - k] with rot(m) = exp(-2 pi i ((fw m D) mod 2^32) / 2^32), one rotation
 *      per output, in float32.  The sum's order is fixed: four partial sums a_j over the k = j
 *      (mod 4) in ascending k, each step two fused multiply-adds per component (re: a.re + c.re
 *      x.re, then - c.im x.im; im: a.im + c.re x.im, then + c.im x.re), then (a_0 + a_1) + (a_2 +
 *      a_3).  |y - y_exact| <= (T + 32) 2^-24 sum|h| max|x|.
 * zfft_tap_push_device is enqueued on its stream with no sync, ordered after earlier work on that
 * stream and after the plan's earlier calls on any stream; d_out must hold the sum of
 * zfft_tap_counts and overlap neither d_iq nor itself across taps.  zfft_tap_open uploads the
 * tap's table on the plan's stream behind the enqueued pushes (it waits on the host only when the
 * same slot is opened again while the plan's enqueued work, its last upload included, is still pending); zfft_tap_close is host
 * bookkeeping.  Every zfft_tap_* call on a plan with taps off returns ZFFT_EINVAL (zfft_tap_shape
 * after reporting 0, 0).  With zfft_plan_timing on a push reports its launch as "tap_push". */
/* max_taps = max_len = 0: off, frees everything.  Otherwise max_taps in [1, 64], max_len in
 * [1, 2048]; anything else ZFFT_EINVAL.  A call closes every tap and restarts the count at 0. */
int zfft_plan_taps(zfft_plan *plan, int32_t max_taps, int32_t max_len);
int zfft_tap_shape(const zfft_plan *plan, int32_t *max_taps, int32_t *max_len);
/* h: n_taps host floats.  Opening an open slot replaces its tap (n_open = the count now). */
int zfft_tap_open(zfft_plan *plan, int32_t slot, int64_t freq_word, int32_t decim, int32_t n_taps, const float *h);
int zfft_tap_close(zfft_plan *plan, int32_t slot); /* ZFFT_EINVAL if the slot is not open */
/* a closed slot reports is_open 0 and zeros; group_delay = (n_taps - 1) / 2 input samples */
int zfft_tap_info(const zfft_plan *plan, int32_t slot, int32_t *is_open, int64_t *freq_word, int32_t *decim,
                  int32_t *n_taps, uint64_t *n_open, double *group_delay);
/* counts[max_taps]: what a push of n_samples (0 .. 2^31 - 1) now would emit per slot (closed: 0);
 * a pure host function of the plan's count and its open taps */
int zfft_tap_counts(const zfft_plan *plan, int64_t n_samples, int64_t *counts);
/* n_samples (1 .. 2^31 - 1; 0 is ZFFT_OK and does nothing) samples of the plan's in_dtype on the
 * device; `stream` is a hipStream_t like every hip_stream of this header (its ordering case, behind
 * a stalled stream, is in tests/test_gpu_tap.py) */
int zfft_tap_push_device(zfft_plan *plan, const void *d_iq, int64_t n_samples, void *d_out, void *stream);
/* host samples and outputs; counts_out[max_taps] (or NULL) as zfft_tap_counts before the push; synchronous */
int zfft_tap_push(zfft_plan *plan, const void *iq, int64_t n_samples, void *out, int64_t *counts_out);
int zfft_tap_state(zfft_plan *plan, uint64_t *samples_seen);
int zfft_tap_reset(zfft_plan *plan, int64_t n0);
/* No plan, no GPU.  A Kaiser-windowed sinc in float64 normalised to unit gain at DC, cutoff in
 * cycles per input sample (0 < cutoff < 0.5), n_taps in [1, 2048], beta >= 0:
 * scipy.signal.firwin(n_taps, 2 cutoff, window=("kaiser", beta)). */
int zfft_tap_design(int32_t n_taps, double cutoff, double beta, double *h_out);
/* No plan, no GPU.  Rule 7's c[k] as n_taps interleaved (re, im) float32 pairs. */
int zfft_tap_table(int64_t freq_word, int32_t n_taps, const float *h, float *c_out);

/* Channeliser: a polyphase-FFT bank of M uniform channels on the samples the plan is given.  Where
 * a tap takes one signal out of the input, the bank takes every channel of the band at once: one
 * prototype low-pass shared by all channels and one M-point transform per output step.  Off by
 * default: a plan that never calls zfft_plan_chan allocates and launches nothing.  The rule
 * (reference: tests/chan_ref.py):
 *   1. samples: the plan counts input samples n = 0, 1, ... from zfft_plan_chan, or from
 *      zfft_chan_reset(plan, n0), which restarts the count at n0 (0 <= n0 <= 2^62) and zeroes the
 *      carry.  x[n] is the input as the plan's in_dtype loader defines it in float32 (all four
 *      in_dtype values), and x[n] = 0 for the samples before the start.  flip_input = 1 has no
 *      continuous time axis: zfft_plan_chan returns ZFFT_EUNSUPPORTED.  The count and the carry
 *      are the channeliser's own, independent of the taps'; a caller who resets both to the same
 *      n0 gets phase-coherent outputs from both.
 *   2. shape: M channels, a power of two in [8, 1024]; P >= 1 taps per branch; T = M P <= 2048
 *      real float32 prototype taps h[0 .. T); decimation D = M (critically sampled) or M / 2
 *      (2x oversampled).
 *   3. outputs: for every step m with m D >= the start and every channel c in [0, M),
 *        y[m, c] = sum_{k < T} h[k] x[m D - k] exp(-2 pi i c (m D - k) / M),
 *      which is a tap at freq_word c 2^32 / M, decimation D, taps h, on the same count.  Channels
 *      c >= M / 2 are the negative frequencies.  Computed in the polyphase form: w_m[s] = sum of
 *      h[k] x[m D - k] over the k with (m D - k) = s (mod M), k ascending -- P terms, each one
 *      fused multiply-add per component from zero -- and y[m, .] = DFT_M(w_m), forward and
 *      unnormalised.  The transform is indexed by the absolute sample index mod M: no per-step
 *      rotation for either D.
 *   4. a push of n_samples at count n0 emits the steps m with n0 <= m D < n0 + n_samples:
 *      ceil((n0 + n_samples) / D) - ceil(n0 / D) of them (zfft_chan_steps, for the next push).
 *      The outputs do not depend on how the stream is cut into pushes, bit for bit: the plan
 *      carries the last T - 1 samples as the loader's float32 values, and the order of the FIR and
 *      the transform are fixed functions of M, P and D.
 *   5. selection: zfft_chan_select(plan, c_first, c_count) keeps the channels (c_first + i) mod M,
 *      i < c_count, 1 <= c_count <= M; the default 0, M is all of them and M / 2, M is ascending
 *      frequency.
 *   6. layout: time-major complex64, out[j K + i] for step j of the push and kept channel i,
 *      K = c_count; one channel's stream is the strided column.  Only kept channels are written,
 *      and a kept channel's values are bit-identical whatever else is selected.
 *   7. the group delay (T - 1) / 2 input samples is reported (zfft_chan_info), not compensated;
 *      the output rate is fs / D.
 *   8. |y - y_exact| <= (P + 5 log2 M + 2) 2^-24 sum|h| max|x|: P rounded multiply-adds per
 *      branch, and per radix-2-equivalent level of the transform a complex multiply, a twiddle
 *      rounded once from float64 and an add.
 *   9. the default prototype is zfft_chan_design(M, P, beta) = zfft_tap_design(M P, 0.5 / M, beta):
 *      a Kaiser sinc, -6 dB at the channel edge, unit gain at DC; beta = 8 where h is NULL.
 * zfft_chan_push_device is enqueued on its stream with no sync, ordered after earlier work on that
 * stream and after the plan's earlier calls on any stream; d_out must hold zfft_chan_steps x
 * c_count complex64 and not overlap d_iq.  Every zfft_chan_* call on a plan with the channeliser
 * off returns ZFFT_EINVAL ("channels are off"; zfft_chan_shape after reporting zeros).  With
 * zfft_plan_timing on a push reports its one launch as "chan_push". */
/* n_chan = 0: off, frees everything.  Otherwise n_chan, taps_per_chan, decim as rule 2, anything
 * else ZFFT_EINVAL; h: n_chan taps_per_chan host floats, or NULL for rule 9's default.  A call
 * restarts the count at 0 with all channels selected. */
int zfft_plan_chan(zfft_plan *plan, int32_t n_chan, int32_t taps_per_chan, int32_t decim, const float *h);
int zfft_chan_shape(const zfft_plan *plan, int32_t *n_chan, int32_t *taps_per_chan, int32_t *decim,
                    int32_t *c_first, int32_t *c_count);
int zfft_chan_select(zfft_plan *plan, int32_t c_first, int32_t c_count);
/* the steps a push of n_samples (0 .. 2^31 - 1) now would emit; a pure host function of the count */
int zfft_chan_steps(const zfft_plan *plan, int64_t n_samples, int64_t *steps);
/* n_samples (1 .. 2^31 - 1; 0 is ZFFT_OK and does nothing) samples of the plan's in_dtype on the device */
int zfft_chan_push_device(zfft_plan *plan, const void *d_iq, int64_t n_samples, void *d_out, void *stream);
/* host samples and outputs; steps_out (or NULL) as zfft_chan_steps before the push; synchronous */
int zfft_chan_push(zfft_plan *plan, const void *iq, int64_t n_samples, void *out, int64_t *steps_out);
int zfft_chan_state(zfft_plan *plan, uint64_t *samples_seen);
int zfft_chan_reset(zfft_plan *plan, int64_t n0);
/* group_delay = (M P - 1) / 2 input samples; rate_ratio = 1 / D output samples per input sample */
int zfft_chan_info(const zfft_plan *plan, double *group_delay, double *rate_ratio);
/* No plan, no GPU.  Rule 9: n_chan taps_per_chan float64 values. */
int zfft_chan_design(int32_t n_chan, int32_t taps_per_chan, double beta, double *h_out);

/* Demodulator bank: AM, FM, SSB and power audio out of complex baseband streams on the device --
 * what the channeliser and the taps emit.  K streams are detected and low-pass filtered at once by
 * one shared real audio FIR with an integer decimation; in the power mode the result is the
 * zero-span trace, power against time on one frequency, with the audio filter as video filter.
 * Off by default: a plan that never calls zfft_plan_demod allocates and launches nothing.  The
 * rule (reference: tests/demod_ref.py):
 *   0. input: complex64 on the device with two strides in complex samples, stream s at step n is
 *      x[n step_stride + s stream_stride], s < K, 1 <= K <= 1024.  zfft_chan_push_device's output
 *      is (step_stride, stream_stride) = (K, 1); one tap's output is (1, anything); `count` taps of
 *      equal decimation written back to back are (1, count).  Nothing is copied or transposed.
 *      step_stride in [1, 2^31], stream_stride in [1, 2^31] (K = 1: [0, 2^31]).
 *   1. count: the bank counts steps n = 0, 1, ... from zfft_plan_demod, or from
 *      zfft_demod_reset(plan, n0), which restarts the count at n0 (0 <= n0 <= 2^62) and zeroes the
 *      carry; x_s[n] = 0 before the start.  The count and the carry are the bank's own,
 *      independent of the taps' and the channeliser's.
 *   2. stream parameters: every stream has a mode and a bfo_word in [-2^31, 2^31), both AM and 0
 *      after zfft_plan_demod, set between pushes by zfft_demod_mode(plan, s_first, s_count, mode,
 *      bfo_word) in stream order.  The detected value d_s[n] is a pure function of x = x_s[n],
 *      p = x_s[n - 1], n and the stream's mode when the push runs, in float32 with every product,
 *      fused multiply-add and square root rounded once:
 *        ZFFT_DEMOD_AM     d = sqrt(fma(x.re, x.re, x.im x.im));
 *        ZFFT_DEMOD_FM     z = x conj(p): z.re = fma(x.re, p.re, x.im p.im), z.im = fma(x.im, p.re,
 *                          -(x.re p.im)); d = atan2f(z.im, z.re) float32(1 / pi), and d = 0 where
 *                          z.re = z.im = 0.  +-1 is +-half the stream's rate;
 *        ZFFT_DEMOD_SSB    d = Re(x r) = fma(x.re, r.re, -(x.im r.im)), r = exp(+2 pi i ((bfo_word
 *                          n) mod 2^32) / 2^32) in float32 from the integer phase (the taps' rot).
 *                          A positive word is USB and a negative one LSB, for a stream centred
 *                          |bfo| off the suppressed carrier;
 *        ZFFT_DEMOD_POWER  d = fma(x.re, x.re, x.im x.im).
 *      A mode change therefore applies to the whole carried window and needs no flush.
 *   3. audio: one real float32 FIR g[0 .. Ta), 1 <= Ta <= 1024, and a decimation Da, 1 <= Da <= 64,
 *      shared by the bank: a[m, s] = sum_{k < Ta} g[k] d_s[m Da - k] for every m with m Da >= the
 *      start.  The sum's order is fixed: four partial sums a_j over the k = j (mod 4) in
 *      ascending k, one fused multiply-add each, then (a_0 + a_1) + (a_2 + a_3).  A push of
 *      `steps` at count n0 emits the m with n0 <= m Da < n0 + steps: ceil((n0 + steps) / Da) -
 *      ceil(n0 / Da) of them (zfft_demod_steps, for the next push).  Output is time-major
 *      float32, out[j K + s] for output j of the push.
 *   4. carry: the bank carries the last Ta complex inputs of every stream on the device, and the
 *      outputs are the same bit for bit however the stream is cut into pushes and whichever form
 *      of the kernel runs (the strides choose it).
 *   5. the group delay (Ta - 1) / 2 steps is reported (zfft_demod_info), not compensated; the
 *      output rate is the streams' rate / Da.  zfft_demod_design is zfft_tap_design; g = NULL
 *      means its 8 Da + 1 taps at cutoff 0.4 / Da, beta 8.  AM's d carries the carrier as a
 *      constant: a band-pass g that removes it is the caller's choice of g.
 *   6. |a - a_exact| <= (Ta + 32) 2^-24 sum|g| max|d| + sum|g| eps_mode.  The first term is the
 *      filter's: each partial sum is at most ceil(Ta / 4) rounded multiply-adds, two adds join
 *      them, and (Ta / 4 + 2) 2^-24 sum|g d| is below it.  The second carries the detector's error
 *      |d - d_exact| <= eps_mode through the filter:
 *        AM     3 2^-24 max|x|: the product and the fma are two roundings of |x|^2, which the
 *               root halves, and the root's own;
 *        POWER  3 2^-24 max|x|^2: the same two roundings, second order included;
 *        SSB    8 2^-24 max|x|: r's components are sincospi within 2 ulp and one fma of the
 *               small-angle step, 4 2^-24 each, 4 sqrt 2 2^-24 |x| in d; the product and the fma
 *               of d add 2 2^-24 |x|;
 *        FM     ZFFT_DEMOD_EPS_FM 2^-24, in units of d (pi radians): the two components of z cost
 *               about 3 2^-24 rad and the device library's atan2f a few units in its last place.
 *               That last figure is measured, not derived: twice the worst |d - d_exact| of the
 *               first run on the device, rounded up (profiles/demod/README.md).  FM has its
 *               branch at +-1: the bound holds for |arg z| <= 0.9 pi.
 * zfft_demod_push_device is enqueued on its stream with no sync, ordered after earlier work on
 * that stream and after the plan's earlier calls on any stream, zfft_demod_mode's included; d_out
 * must hold zfft_demod_steps x K float32 and not overlap d_x.  Every zfft_demod_* call on a plan
 * with the bank off returns ZFFT_EINVAL ("demod is off"; zfft_demod_shape after reporting zeros).
 * With zfft_plan_timing on a push reports its one launch as "demod_push". */
enum { ZFFT_DEMOD_AM = 0, ZFFT_DEMOD_FM = 1, ZFFT_DEMOD_SSB = 2, ZFFT_DEMOD_POWER = 3 };
#define ZFFT_DEMOD_EPS_FM 3
/* n_streams = 0: off, frees everything.  Otherwise n_streams, n_taps, decim as rules 0 and 3,
 * anything else ZFFT_EINVAL; g: n_taps host floats, or NULL for rule 5's default, with n_taps 0 or
 * 8 decim + 1.  A call restarts the count at 0 with every stream at AM. */
int zfft_plan_demod(zfft_plan *plan, int32_t n_streams, int32_t n_taps, int32_t decim, const float *g);
int zfft_demod_shape(const zfft_plan *plan, int32_t *n_streams, int32_t *n_taps, int32_t *decim);
/* streams [s_first, s_first + s_count) to `mode` (ZFFT_DEMOD_*) and bfo_word (used by SSB alone) */
int zfft_demod_mode(zfft_plan *plan, int32_t s_first, int32_t s_count, int32_t mode, int64_t bfo_word);
/* the outputs a push of `steps` (0 .. 2^31 - 1) now would emit; a pure host function of the count */
int zfft_demod_steps(const zfft_plan *plan, int64_t steps, int64_t *outputs);
/* steps (1 .. 2^31 - 1; 0 is ZFFT_OK and does nothing) of the K streams on the device, rule 0 */
int zfft_demod_push_device(zfft_plan *plan, const void *d_x, int64_t steps, int64_t step_stride,
                           int64_t stream_stride, void *d_out, void *stream);
/* host input ((steps - 1) step_stride + (K - 1) stream_stride + 1 complex64) and outputs;
 * outputs_out (or NULL) as zfft_demod_steps before the push; synchronous */
int zfft_demod_push(zfft_plan *plan, const void *x, int64_t steps, int64_t step_stride, int64_t stream_stride,
                    void *out, int64_t *outputs_out);
int zfft_demod_state(zfft_plan *plan, uint64_t *steps_seen);
int zfft_demod_reset(zfft_plan *plan, int64_t n0);
/* group_delay = (Ta - 1) / 2 steps; rate_ratio = 1 / Da outputs per step */
int zfft_demod_info(const zfft_plan *plan, double *group_delay, double *rate_ratio);
/* No plan, no GPU.  zfft_tap_design for n_taps in [1, 1024]. */
int zfft_demod_design(int32_t n_taps, double cutoff, double beta, double *h_out);

/* Resampler bank: K real float32 lanes on the device at L / M times their rate -- the
 * demodulator's audio at a rate a sound device takes, or a complex stream (two lanes) at the rate
 * a decoder wants -- as float32 or as int16 PCM.  Off by default: a plan that never calls
 * zfft_plan_resamp allocates and launches nothing.  The rule (reference: tests/resamp_ref.py):
 *   0. input: float32 on the device, time-major: lane s at step n is x[n step_stride + s], s < K,
 *      1 <= K <= 2048, step_stride in floats in [K, 2^31].  zfft_demod_push_device's output is
 *      (K, step_stride) = (streams, streams).  A complex stream is two lanes: one tap's output is
 *      K = 2, step_stride = 2, the channeliser's (steps, channels) complex64 is K = step_stride =
 *      2 channels.  Nothing is copied or transposed: a subset of neighbouring lanes is read in
 *      place by offsetting the pointer and keeping the stride.
 *   1. ratio: L outputs per M inputs, 1 <= L <= 512, 1 <= M <= 4096, gcd(L, M) = 1 (anything else
 *      is ZFFT_EINVAL); T taps per phase, 1 <= T <= 128, L T <= 8192; one real float32 prototype
 *      h[0 .. T L) at the upsampled rate, shared by all lanes.
 *   2. count: the bank counts input steps n = 0, 1, ... from zfft_plan_resamp, or from
 *      zfft_resamp_reset(plan, n0), which restarts the count at n0 (0 <= n0 <= 2^62) and zeroes the
 *      carry; x_s[n] = 0 before the start.  The count and the carry are the bank's own, independent
 *      of the taps', the channeliser's and the demodulator's.  Output m sits at input time m M / L:
 *      its input index is i_m = floor(m M / L), its phase p_m = m M mod L, and
 *        y[m, s] = sum_{k < T} h[k L + p_m] x_s[i_m - k]
 *      -- scipy.signal.upfirdn(h, x, L, M) on an absolute time axis.  The sum's order is fixed:
 *      four partial sums a_j over the k = j (mod 4) in ascending k, one fused multiply-add each,
 *      then (a_0 + a_1) + (a_2 + a_3).  Exactly T products are formed per output.
 *   3. push: a push of `steps` at count n0 emits the m with n0 <= i_m < n0 + steps:
 *      ceil((n0 + steps) L / M) - ceil(n0 L / M) of them (zfft_resamp_steps, for the next push; a
 *      pure host function in 128-bit arithmetic, n0 L reaching 2^71).  Output is time-major,
 *      out[j K + s] for output j of the push.
 *   4. format: ZFFT_RESAMP_F32 writes y.  ZFFT_RESAMP_S16 writes the int16
 *      q = clamp(rint(y scale), -32768, 32767): one rounded float32 product with the float32
 *      `scale` of the enable (32767 is the usual one, for |y| <= 1), rint to nearest with ties to
 *      even; NaN gives 0 and +-inf saturate.
 *   5. carry: the bank carries the last T - 1 input steps of every lane on the device, and the
 *      outputs are the same bit for bit however the stream is cut into pushes, pushes shorter than
 *      the carry included, and whichever form of the kernel runs.
 *   6. the group delay (T L - 1) / (2 L) input steps and the rate ratio L / M are reported
 *      (zfft_resamp_info), not compensated.  zfft_resamp_design(L, M, T, beta, h_out) is
 *      zfft_tap_design's formula at length T L and cutoff 0.4 / max(L, M) cycles per upsampled
 *      sample -- a symmetric Kaiser sinc of unit sum -- multiplied by L, so that every phase has
 *      unit gain.  h = NULL means that design with T = 16 ceil(max(L, M) / L) and beta 8; where
 *      that T breaks rule 1 the call is ZFFT_EINVAL and the caller gives taps.
 *   7. |y - y_exact| <= (T + 32) 2^-24 sum_k |h[k L + p]| max|x|: each partial sum is at most
 *      ceil(T / 4) rounded multiply-adds and two adds join them (rule 6 of the demodulator with
 *      no detector term).  S16 adds half a code, and one rounding of the product.
 * zfft_resamp_push_device is enqueued on its stream with no sync, ordered after earlier work on
 * that stream and after the plan's earlier calls on any stream; d_out must hold zfft_resamp_steps x
 * K elements of the format and not overlap d_x.  Every zfft_resamp_* call on a plan with the bank
 * off returns ZFFT_EINVAL ("resamp is off"; zfft_resamp_shape after reporting zeros).  With
 * zfft_plan_timing on a push reports its one launch as "resamp_push". */
enum { ZFFT_RESAMP_F32 = 0, ZFFT_RESAMP_S16 = 1 };
/* n_lanes = 0: off, frees everything.  Otherwise n_lanes, L, M, taps_per_phase as rules 0 and 1,
 * anything else ZFFT_EINVAL; h: L taps_per_phase host floats, or NULL for rule 6's default, with
 * taps_per_phase 0 or 16 ceil(max(L, M) / L); format ZFFT_RESAMP_*, scale used by S16 alone.  A
 * call restarts the count at 0. */
int zfft_plan_resamp(zfft_plan *plan, int32_t n_lanes, int32_t L, int32_t M, int32_t taps_per_phase, const float *h,
                     int32_t format, float scale);
int zfft_resamp_shape(const zfft_plan *plan, int32_t *n_lanes, int32_t *L, int32_t *M, int32_t *taps_per_phase,
                      int32_t *format);
/* the outputs a push of `steps` (0 .. 2^31 - 1) now would emit; a pure host function of the count */
int zfft_resamp_steps(const zfft_plan *plan, int64_t steps, int64_t *outputs);
/* steps (1 .. 2^31 - 1; 0 is ZFFT_OK and does nothing) of the K lanes on the device, rule 0 */
int zfft_resamp_push_device(zfft_plan *plan, const void *d_x, int64_t steps, int64_t step_stride, void *d_out,
                            void *stream);
/* host input ((steps - 1) step_stride + K float32) and outputs; outputs_out (or NULL) as
 * zfft_resamp_steps before the push; synchronous */
int zfft_resamp_push(zfft_plan *plan, const void *x, int64_t steps, int64_t step_stride, void *out,
                     int64_t *outputs_out);
int zfft_resamp_state(zfft_plan *plan, uint64_t *steps_seen);
int zfft_resamp_reset(zfft_plan *plan, int64_t n0);
/* group_delay = (T L - 1) / (2 L) input steps; rate_ratio = L / M outputs per step */
int zfft_resamp_info(const zfft_plan *plan, double *group_delay, double *rate_ratio);
/* No plan, no GPU.  Rule 6: L taps_per_phase float64 values. */
int zfft_resamp_design(int32_t L, int32_t M, int32_t taps_per_phase, double beta, double *h_out);

/* Level bank: look-ahead gain control (AGC), squelch and a level meter on K real float32 lanes on
 * the device -- the link between the demodulator's audio and the resampler's PCM, whose one
 * `scale` cannot serve channels 80 dB apart.  Finite memory and feed-forward on an absolute block
 * grid, not a recursive attack / release filter: every operation is a max, one division, one
 * subtraction, one fused multiply-add and one product, so the outputs do not depend on how the
 * stream is cut.  Off by default: a plan that never calls zfft_plan_level allocates and launches
 * nothing.  The rule (reference and float32 model: tests/level_ref.py):
 *   0. input: float32 on the device, time-major, as the resampler's rule 0: lane s at step n is
 *      x[n step_stride + s], s < K, 1 <= K <= 2048, step_stride in floats in [K, 2^31].
 *      zfft_demod_push_device's output is (K, step_stride) = (streams, streams); a subset of
 *      neighbouring lanes is read in place by offsetting the pointer and keeping the stride.  An
 *      optional key d_key of the same shape with its own key_stride is the side chain: the gains
 *      come from the key, the samples from x (FM audio gated by the same channels' POWER trace from
 *      a second plan's demodulator).  d_key = NULL: the key is x.
 *   1. parameters: block length B, a power of two in [8, 1024]; hold H in blocks, in [0, 4096];
 *      float32 target, gmax, floor, each in [2^-60, 2^60]; float32 squelch, 0 (off) or in
 *      [2^-60, 2^60].  Anything else is ZFFT_EINVAL.
 *   2. count: the bank counts steps n = 0, 1, ... from zfft_plan_level, or from
 *      zfft_level_reset(plan, n0), which restarts the count at n_r = n0 (0 <= n0 <= 2^62) and
 *      zeroes the carry.  Block b is the steps [b B, (b + 1) B) of that absolute axis.  x and the
 *      key are 0 before n_r, so every block before the start has peak 0.  The count and the carry
 *      are the bank's own.
 *   3. block peak: P[b, s] = max over the block of m(key_s[n]), m(v) = 0 where v is NaN, else
 *      min(|v|, 2^60).  With this cap and rule 1's ranges no gain is denormal, or zero by underflow.
 *   4. envelope and block gain: E[b, s] = max(P[b - H .. b, s]);
 *      G[b, s] = min(gmax, target / max(E, floor)) in float32, the division correctly rounded;
 *      G = 0 where squelch > 0 and E < squelch.  (A fixed gain c with squelch alone: gmax = c,
 *      target = 2^60.)
 *   5. step gain: for n = b B + i, g_lo = min(G[b - 1], G[b]), g_hi = min(G[b], G[b + 1]),
 *      d = g_hi - g_lo rounded once, g = fma(float32(i) / B, d, g_lo); i / B is exact.  The gain
 *      ramps down during the block before a louder one (the look-ahead attack), up during the
 *      first block after the hold ends, and within block b never exceeds G[b] but for rounding.
 *   6. output: y[n, s] = g x_s[n], one rounded product; time-major, out[j K + s] for emitted step
 *      j of the push.  A NaN sample is NaN in its own output and nowhere else; an infinity counts
 *      as 2^60 in the peak and is itself +-inf, or NaN where g = 0.  For finite |x| <= 2^60,
 *      |y| <= target (1 + 2^-21): with the key x, |x_s[n]| <= P[b] <= E[b], and the exact ramp lies
 *      between g_lo and g_hi, both at most G[b]; four roundings of at most 2^-24 each stand between
 *      target / E[b] and y -- the division, d (an error of at most 2^-24 G[b] in g), the fma and the
 *      product -- and (1 + 2^-24)^4 < 1 + 2^-21.
 *   7. push: block b can be emitted once block b + 1 is complete.  With
 *      emitted(N) = max(n_r, B (floor(N / B) - 1)), a push of `steps` at count n0 emits the steps
 *      [emitted(n0), emitted(n0 + steps)) (zfft_level_steps, for the next push; a pure host
 *      function).  The latency is between B and 2 B - 1 steps (zfft_level_info), not compensated.
 *      To end a stream push 2 B zeros.
 *   8. carry: per lane the bank carries the at most 2 B - 1 unemitted steps of x, the running peak
 *      of the incomplete block and the peaks of the last H + 2 complete blocks (H + 3 values: what
 *      the next emitted blocks still need), all on the device.  The outputs are the same
 *      bit for bit however the stream is cut into pushes, pushes shorter than the carry and pushes
 *      that emit nothing included, and whichever form of the kernels runs.
 *   9. meter: zfft_level_meter(plan, env_out, gain_out) is synchronous and returns K floats each:
 *      E and G of the newest complete block of every lane; before any block is complete E = 0 and
 *      G is rule 4's for E = 0.  The bank's S-meter, and "which channels are open" (G > 0).
 * zfft_level_push_device is enqueued on its stream with no sync, ordered after earlier work on
 * that stream and after the plan's earlier calls on any stream (a push longer than any before
 * first grows the bank's work arrays, which waits); d_out must hold zfft_level_steps x K floats
 * and not overlap d_x or d_key.  Every zfft_level_* call on a plan with the bank off returns
 * ZFFT_EINVAL ("level is off"; zfft_level_shape after reporting zeros).  With zfft_plan_timing on a
 * push reports its launches as "level_peaks", "level_gains" (where it emits) and "level_apply". */
/* n_lanes = 0: off, frees everything.  Otherwise n_lanes, block, hold, target, gmax, floor and
 * squelch as rules 0 and 1, anything else ZFFT_EINVAL.  A call restarts the count at 0. */
int zfft_plan_level(zfft_plan *plan, int32_t n_lanes, int32_t block, int32_t hold, float target, float gmax, float floor,
                    float squelch);
int zfft_level_shape(const zfft_plan *plan, int32_t *n_lanes, int32_t *block, int32_t *hold, float *target, float *gmax,
                     float *floor, float *squelch);
/* the steps a push of `steps` (0 .. 2^31 - 1) now would emit; a pure host function of the count */
int zfft_level_steps(const zfft_plan *plan, int64_t steps, int64_t *outputs);
/* steps (1 .. 2^31 - 1; 0 is ZFFT_OK and does nothing) of the K lanes on the device, rule 0;
 * d_key NULL (key_stride ignored) or the key */
int zfft_level_push_device(zfft_plan *plan, const void *d_x, int64_t steps, int64_t step_stride, const void *d_key,
                           int64_t key_stride, void *d_out, void *stream);
/* host input ((steps - 1) step_stride + K float32), key (NULL, or the same shape and stride) and
 * outputs; outputs_out (or NULL) as zfft_level_steps before the push; synchronous */
int zfft_level_push(zfft_plan *plan, const void *x, const void *key, int64_t steps, int64_t step_stride, void *out,
                    int64_t *outputs_out);
int zfft_level_state(zfft_plan *plan, uint64_t *steps_seen);
int zfft_level_reset(zfft_plan *plan, int64_t n0);
/* latency_min = B and latency_max = 2 B - 1 steps; rate_ratio = 1 output per step */
int zfft_level_info(const zfft_plan *plan, double *latency_min, double *latency_max, double *rate_ratio);
/* rule 9: K floats each; synchronous */
int zfft_level_meter(zfft_plan *plan, float *env_out, float *gain_out);

const char *zfft_last_error(void);
int zfft_device_count(void);
int zfft_version(void);

#ifdef __cplusplus
}
#endif

#endif /* ZFFT_H */
