// zfft_waterfall.cpp -- the waterfall of libzfft.so: the ring of rows, colormaps, rendering,
// autolevel and the page-locked host buffers of the display entry points (C-ABI, zfft.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "zfft.h"
#include "zfft_plan.h"

using namespace zfft;

namespace {

// ---- waterfall colormaps (Waterfall.Colors / lookuptable, S:1580-1585, 1613-1623) ----
// pg.ColorMap(pos, color).getLookupTable(0.0, 1.0, 256): x = linspace(0, 1, 256), each
// channel np.interp(x, pos, color), truncated to uint8; the maps are opaque, so the LUT has
// no alpha channel and makeARGB draws alpha 255.  'Default' keeps the reference's stop
// value 2020 as a numpy < 2 uint8 array stored it (2020 mod 256 = 228).
struct ColorStops {
  const char *name;
  int n;
  double pos[6];
  int rgba[6][4];
};
const ColorStops kColormaps[] = {
    {"Default", 3, {0.0, 0.4, 1.0}, {{0, 0, 90, 255}, {200, 2020 % 256, 0, 255}, {255, 0, 0, 255}}},
    {"Matrix", 2, {0.0, 1.0}, {{0, 0, 0, 255}, {0, 255, 0, 255}}},
    {"Red Green", 3, {0.0, 0.5, 1.0}, {{0, 0, 0, 255}, {0, 255, 0, 255}, {255, 0, 0, 255}}},
    {"Tropical", 6, {0.0, 0.2, 0.4, 0.6, 0.8, 1.0},
     {{68, 40, 153, 255}, {222, 68, 252, 255}, {252, 38, 99, 255}, {252, 181, 38, 255},
      {86, 235, 49, 255}, {3, 71, 7, 255}}},
};

// np.interp(x, xp, fp) for increasing xp (numpy/core/src/multiarray/compiled_base.c)
double np_interp(double x, const double *xp, const double *fp, int n) {
  if (x <= xp[0]) return fp[0];
  if (x >= xp[n - 1]) return fp[n - 1];
  int j = 0;
  while (j + 1 < n && xp[j + 1] <= x) ++j;
  if (x == xp[j]) return fp[j];
  const double slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
  return slope * (x - xp[j]) + fp[j];
}

void build_lut(const char *name, uint8_t *lut) {
  const ColorStops *cm = &kColormaps[0];  // any other name -> 'Default' (S:1613-1614)
  for (const ColorStops &c : kColormaps)
    if (name && std::strcmp(name, c.name) == 0) cm = &c;
  const double step = 1.0 / 255.0;  // np.linspace(0, 1, 256): arange * step, last = stop
  for (int i = 0; i < 256; ++i) {
    const double x = i == 255 ? 1.0 : (double)i * step;
    for (int ch = 0; ch < 3; ++ch) {
      double fp[6];
      for (int k = 0; k < cm->n; ++k) fp[k] = (double)cm->rgba[k][ch];
      lut[4 * i + ch] = (uint8_t)np_interp(x, cm->pos, fp, cm->n);  // astype(ubyte): truncation
    }
    lut[4 * i + 3] = 255;
  }
}

int ensure_waterfall(zfft_plan *p) {
  const int W = p->cfg.n_win;
  if (p->wf_ready && p->W == W) return ZFFT_OK;
  if (W < 10 || (p->cfg.scroll > 0 && W / 4 < 15) || (p->cfg.scroll < 0 && W / 4 < 10))
    return fail(ZFFT_EINVAL, "waterfall needs n_win >= 60 (scroll=+1) or >= 40 (scroll=-1): "
                             "Waterfall.image_update indexes rows 5..14 / -10..-3 (S:1655-1662)");
  const int H = W / 4;
  hipError_t e = p->ring.ensure((size_t)H * W * sizeof(float));
  if (e == hipSuccess) e = p->img.ensure((size_t)H * W * sizeof(float));
  if (e == hipSuccess) e = p->one_row.ensure((size_t)W * sizeof(float));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "waterfall allocation failed");
  int rc = use_stream(p, p->stream);
  if (rc) return rc;
  e = launch_waterfall_init(p->ring.as<float>(), H, W, p->stream);
  if (e != hipSuccess) return hip_fail(e, "waterfall init");
  rc = done_on(p, p->stream);
  if (rc) return rc;
  p->H = H;
  p->W = W;
  p->off = 0;
  p->wf_ready = true;
  return ZFFT_OK;
}

}  // namespace

extern "C" {

int zfft_waterfall_shape(const zfft_plan *p, int32_t *rows, int32_t *cols) {
  if (!p || !rows || !cols) return fail(ZFFT_EINVAL, "null argument");
  *rows = p->cfg.n_win / 4;
  *cols = p->cfg.n_win;
  return ZFFT_OK;
}

int zfft_waterfall_reset(zfft_plan *p, int32_t scroll) {
  int rc = enter(p);
  if (rc) return rc;
  if (scroll != 1 && scroll != -1) return fail(ZFFT_EINVAL, "scroll must be +1 or -1");
  p->cfg.scroll = scroll;
  p->wf_ready = false;  // init_image on the next push / read (S:2074-2077)
  return ensure_waterfall(p);
}

int zfft_waterfall_push_device(zfft_plan *p, const float *d_rows, int32_t count,
                               void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  if (!d_rows || count < 1) return fail(ZFFT_EINVAL, "bad rows / count");
  rc = ensure_waterfall(p);
  if (rc) return rc;
  hipStream_t st = pick_stream(p, hip_stream);
  rc = use_stream(p, st);  // after the ring init and the rows' producer, on any stream
  if (rc) return rc;
  hipError_t e = launch_waterfall_push(p->ring.as<float>(), p->H, p->W, d_rows, p->W, count,
                                       p->off, p->cfg.scroll, st);
  if (e != hipSuccess) return hip_fail(e, "waterfall push");
  p->off = ((p->off + (int64_t)count * p->cfg.scroll) % p->H + p->H) % p->H;
  return done_on(p, st);
}

int zfft_waterfall_push(zfft_plan *p, const float *row) {
  int rc = enter(p);
  if (rc) return rc;
  rc = ensure_waterfall(p);
  if (rc) return rc;
  const float *src = p->last_row;
  if (row) {
    rc = use_stream(p, p->stream);  // one_row may still be read by the previous push
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(p->one_row.p, row, (size_t)p->W * sizeof(float),
                                  hipMemcpyHostToDevice, p->stream);
    if (e != hipSuccess) return hip_fail(e, "H2D row");
    src = p->one_row.as<float>();
  }
  if (!src) return fail(ZFFT_EINVAL, "no row given and no frame processed yet");
  if (!row && row_length(p) < p->W)  // columns >= row_length were never written
    return fail(ZFFT_EINVAL, "the plan's rows are shorter than n_win (odd n_win, or the one-sided "
                             "real-input crop): img_array[-1:] = psd raises in the reference "
                             "(S:1640); push a full-width row instead");
  rc = zfft_waterfall_push_device(p, src, 1, p->stream);
  if (rc) return rc;
  hipError_t e = hipStreamSynchronize(p->stream);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "sync");
}

int zfft_waterfall_read(zfft_plan *p, float *img_out) {
  int rc = enter(p);
  if (rc) return rc;
  if (!img_out) return fail(ZFFT_EINVAL, "null output");
  rc = ensure_waterfall(p);
  if (rc) return rc;
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = launch_waterfall_read(p->ring.as<float>(), p->H, p->W, p->off, p->img.as<float>(),
                                       p->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(img_out, p->img.p, (size_t)p->H * p->W * sizeof(float),
                       hipMemcpyDeviceToHost, p->stream);
  return sync_read(p, e, "waterfall read");
}

int zfft_colormap_lut(const char *name, uint8_t *lut_rgba) {
  if (!lut_rgba) return fail(ZFFT_EINVAL, "null output");
  build_lut(name, lut_rgba);
  return ZFFT_OK;
}

int zfft_waterfall_colormap(zfft_plan *p, const char *name) {
  int rc = enter(p);
  if (rc) return rc;
  p->cmap = name ? name : "Default";
  p->lut_ready = p->lut_uploaded = false;
  return ZFFT_OK;
}

int zfft_waterfall_levels(zfft_plan *p, double minlev, double maxlev) {
  int rc = enter(p);
  if (rc) return rc;
  if (!std::isfinite(minlev) || !std::isfinite(maxlev)) return fail(ZFFT_EINVAL, "levels must be finite");
  p->lev_lo = minlev;
  p->lev_hi = maxlev;
  return ZFFT_OK;
}

int zfft_waterfall_get_levels(const zfft_plan *p, double *minlev, double *maxlev) {
  if (!p || !minlev || !maxlev) return fail(ZFFT_EINVAL, "null argument");
  *minlev = p->lev_lo;
  *maxlev = p->lev_hi;
  return ZFFT_OK;
}

}  // extern "C"

// The colormap LUT on the device (built and uploaded on first use, on st) and makeARGB's
// levels (pyqtgraph functions.py): equal levels -> max = nextafter(max, 2 max); scale = lut
// size / (max - min) (1 when the range is 0)
int zfft::render_setup(zfft_plan *p, hipStream_t st, double *lo, double *scale) {
  if (!p->lut_ready) {
    build_lut(p->cmap.c_str(), p->lut);
    p->lut_ready = true;
  }
  if (!p->lut_uploaded) {
    hipError_t e = p->lut_d.ensure(sizeof(p->lut));
    if (e == hipSuccess) e = hipMemcpyAsync(p->lut_d.p, p->lut, sizeof(p->lut), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return hip_fail(e, "LUT upload");
    p->lut_uploaded = true;
  }
  double l = p->lev_lo, h = p->lev_hi;
  if (l == h) h = std::nextafter(h, 2.0 * h);
  double rng = h - l;
  if (rng == 0.0) rng = 1.0;
  *lo = l;
  *scale = 256.0 / rng;
  return ZFFT_OK;
}

namespace {
// zfft_waterfall_push_render / _push_read64: count host rows pushed, then the image emitted
// (RGBA8 or float64) and copied to the host -- one kernel for the per-line case, one copy, one
// wait.  The rows are staged in page-locked memory the kernels read in place.
int push_emit(zfft_plan *p, const float *rows, int32_t count, bool f64, void *host_out) {
  int rc = enter(p);
  if (rc) return rc;
  if (!host_out) return fail(ZFFT_EINVAL, "null output");
  if (count < 0 || (count > 0 && !rows)) return fail(ZFFT_EINVAL, "bad rows / count");
  rc = ensure_waterfall(p);
  if (rc) return rc;
  const int H = p->H, W = p->W;
  const size_t npx = (size_t)H * W, bytes = npx * (f64 ? sizeof(double) : 4);
  hipError_t e = f64 ? p->img64.ensure(bytes) : p->rgba.ensure(bytes);
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "image buffer allocation failed");
  const float *drows = nullptr;
  if (count > 0) {
    rc = pin_rows(p, rows, (size_t)count * W * sizeof(float), &drows);
    if (rc) return rc;
  }
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  double lo = 0.0, scale = 1.0;
  if (!f64) {
    rc = render_setup(p, p->stream, &lo, &scale);
    if (rc) return rc;
  }
  // a small image into page-locked host memory is written by the kernel in place (no copy
  // command: the UI's widths, W <= 1024, are 64 KB .. 1 MB per image); a large one goes through
  // the device buffer and one DMA copy (at W = 8192 the 67 MB RGBA image copies faster so)
  void *dout = f64 ? p->img64.p : p->rgba.p;
  void *hout = nullptr;
  if (bytes <= kDisplayZeroCopyMax && hipHostGetDevicePointer(&hout, host_out, 0) == hipSuccess && hout)
    dout = hout;
  else
    (void)hipGetLastError(), hout = nullptr;
  if (count > 1) {  // the batch through the push kernels, then the image
    e = launch_waterfall_push(p->ring.as<float>(), H, W, drows, W, count, p->off, p->cfg.scroll, p->stream);
    if (e != hipSuccess) return hip_fail(e, "waterfall push");
    p->off = ((p->off + (int64_t)count * p->cfg.scroll) % H + H) % H;
    drows = nullptr;
  }
  e = launch_waterfall_push_emit(p->ring.as<float>(), H, W, p->off, p->cfg.scroll, drows, p->lut_d.p, lo,
                                 scale, dout, f64, p->stream);
  if (e != hipSuccess) return hip_fail(e, "waterfall push + emit");
  if (drows) p->off = ((p->off + p->cfg.scroll) % H + H) % H;
  if (!hout) e = hipMemcpyAsync(host_out, dout, bytes, hipMemcpyDeviceToHost, p->stream);
  return sync_read(p, e, "waterfall image copy");
}
}  // namespace

extern "C" {

int zfft_waterfall_push_render(zfft_plan *p, const float *rows, int32_t count, uint8_t *rgba_out) {
  return push_emit(p, rows, count, false, rgba_out);
}

int zfft_waterfall_push_read64(zfft_plan *p, const float *rows, int32_t count, double *img_out) {
  return push_emit(p, rows, count, true, img_out);
}

int zfft_waterfall_render_device(zfft_plan *p, uint8_t *d_rgba, void *hip_stream) {
  int rc = enter(p);
  if (rc) return rc;
  if (!d_rgba) return fail(ZFFT_EINVAL, "null output");
  rc = ensure_waterfall(p);
  if (rc) return rc;
  hipStream_t st = pick_stream(p, hip_stream);
  rc = use_stream(p, st);
  if (rc) return rc;
  double lo, scale;
  rc = render_setup(p, st, &lo, &scale);
  if (rc) return rc;
  hipError_t e = launch_waterfall_render(p->ring.as<float>(), p->H, p->W, p->off, p->lut_d.p, lo, scale,
                                         d_rgba, st);
  if (e != hipSuccess) return hip_fail(e, "waterfall render");
  return done_on(p, st);
}

int zfft_waterfall_render(zfft_plan *p, uint8_t *rgba_out) {
  int rc = enter(p);
  if (rc) return rc;
  if (!rgba_out) return fail(ZFFT_EINVAL, "null output");
  rc = ensure_waterfall(p);
  if (rc) return rc;
  const size_t bytes = (size_t)p->H * p->W * 4;
  hipError_t e = p->rgba.ensure(bytes);
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "render buffer allocation failed");
  rc = zfft_waterfall_render_device(p, p->rgba.as<uint8_t>(), p->stream);
  if (rc) return rc;
  e = hipMemcpyAsync(rgba_out, p->rgba.p, bytes, hipMemcpyDeviceToHost, p->stream);
  return sync_read(p, e, "render copy");
}

int zfft_host_alloc(size_t bytes, void **out) {
  if (!out || bytes == 0) return fail(ZFFT_EINVAL, "zfft_host_alloc: null output or zero size");
  *out = nullptr;
  hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    *out = nullptr;
    return fail(ZFFT_ENOMEM, "page-locked host allocation failed");
  }
  return ZFFT_OK;
}

int zfft_host_free(void *ptr) {
  if (!ptr) return ZFFT_OK;
  hipError_t e = hipHostFree(ptr);
  return e == hipSuccess ? ZFFT_OK : hip_fail(e, "hipHostFree");
}

int zfft_waterfall_autolevel(zfft_plan *p, double *minlev, double *maxlev) {
  int rc = enter(p);
  if (rc) return rc;
  rc = ensure_waterfall(p);
  if (rc) return rc;
  const int64_t n = (int64_t)p->H * p->W;
  hipError_t e = p->al_hist.ensure(4 * 65536 * sizeof(unsigned));
  if (e == hipSuccess) e = p->al_bins.ensure(4 * sizeof(unsigned));
  if (e != hipSuccess) return fail(ZFFT_ENOMEM, "autolevel workspace allocation failed");
  // pass 1: counts per top-16-bit key of the pixels < 0
  std::vector<unsigned> h1(65536);
  rc = use_stream(p, p->stream);
  if (rc) return rc;
  e = hipMemsetAsync(p->al_hist.p, 0, 65536 * sizeof(unsigned), p->stream);
  if (e == hipSuccess) e = launch_autolevel_hist_hi(p->ring.as<float>(), n, p->al_hist.as<unsigned>(), p->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h1.data(), p->al_hist.p, 65536 * sizeof(unsigned), hipMemcpyDeviceToHost, p->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
  if (e != hipSuccess) return hip_fail(e, "autolevel pass 1");
  int64_t cnt = 0;
  for (unsigned c : h1) cnt += c;
  if (cnt == 0) return fail(ZFFT_EINVAL, "autolevel: no pixel below 0");  // np.percentile of an empty array raises
  // numpy percentile, method 'linear': virtual index (n-1) q, q = p/100; the order
  // statistics at floor and floor+1 (clipped to n-1)
  const double qs[2] = {2.0 / 100.0, 98.0 / 100.0};
  double vi[2];
  int64_t ranks[4];
  for (int k = 0; k < 2; ++k) {
    vi[k] = (double)(cnt - 1) * qs[k];
    const int64_t prev = (int64_t)std::floor(vi[k]);
    ranks[2 * k] = std::min<int64_t>(std::max<int64_t>(prev, 0), cnt - 1);
    ranks[2 * k + 1] = std::min<int64_t>(std::max<int64_t>(prev + 1, 0), cnt - 1);
  }
  // the top bin and the rank inside it of each wanted rank
  unsigned bin_of[4];
  int64_t within[4];
  for (int r = 0; r < 4; ++r) {
    int64_t acc = 0;
    unsigned b = 0;
    while (acc + h1[b] <= ranks[r]) acc += h1[b++];
    bin_of[r] = b;
    within[r] = ranks[r] - acc;
  }
  unsigned bins[4];
  int nb = 0, slot[4];
  for (int r = 0; r < 4; ++r) {
    int j = 0;
    while (j < nb && bins[j] != bin_of[r]) ++j;
    if (j == nb) bins[nb++] = bin_of[r];
    slot[r] = j;
  }
  std::vector<unsigned> h2((size_t)nb * 65536);
  e = hipMemcpyAsync(p->al_bins.p, bins, nb * sizeof(unsigned), hipMemcpyHostToDevice, p->stream);
  if (e == hipSuccess) e = hipMemsetAsync(p->al_hist.p, 0, (size_t)nb * 65536 * sizeof(unsigned), p->stream);
  if (e == hipSuccess)
    e = launch_autolevel_hist_lo(p->ring.as<float>(), n, p->al_bins.as<unsigned>(), nb, p->al_hist.as<unsigned>(), p->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h2.data(), p->al_hist.p, (size_t)nb * 65536 * sizeof(unsigned), hipMemcpyDeviceToHost, p->stream);
  rc = sync_read(p, e, "autolevel pass 2");
  if (rc) return rc;
  double val[4];
  for (int r = 0; r < 4; ++r) {
    const unsigned *hb = h2.data() + (size_t)slot[r] * 65536;
    int64_t acc = 0;
    unsigned lo16 = 0;
    while (acc + hb[lo16] <= within[r]) acc += hb[lo16++];
    const uint32_t key = (bin_of[r] << 16) | lo16;
    uint32_t bits = ~key;  // neg_key inverse
    float f;
    std::memcpy(&f, &bits, 4);
    val[r] = (double)f;
  }
  // numpy _lerp(a, b, t): a + (b - a) t, or b - (b - a)(1 - t) when t >= 0.5
  double lev[2];
  for (int k = 0; k < 2; ++k) {
    const double a = val[2 * k], b = val[2 * k + 1];
    const double t = vi[k] - std::floor(vi[k]);
    const double d = b - a;
    lev[k] = t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
  }
  p->lev_lo = lev[0];
  p->lev_hi = lev[1];
  if (minlev) *minlev = lev[0];
  if (maxlev) *maxlev = lev[1];
  return ZFFT_OK;
}

}  // extern "C"
