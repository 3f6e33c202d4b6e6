// zfft_stream.cpp -- the shared host path of the sample-stream producers (zfft_stream.h).
#include "zfft_stream.h"

#include <string>

#include "zfft_stream_plan.h"

namespace zfft {

int stream_restart(zfft_plan *p, StreamState &s, const StreamNames &nm, uint64_t n0) {
  int rc = use_stream(p, p->stream);
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(s.carry.p, 0, 2 * s.carry_len * sizeof(float2), p->stream);
  if (e != hipSuccess) return hip_fail(e, (std::string(nm.who) + " reset").c_str());
  s.n = n0;
  s.par = 0;
  return done_on(p, p->stream);
}

int stream_reset(zfft_plan *p, StreamState &s, const StreamNames &nm, int64_t n0) {
  if (n0 < 0 || (uint64_t)n0 > kStreamMaxCount) return fail(ZFFT_EINVAL, std::string(nm.who) + "_reset: n0 in [0, 2^62]");
  return stream_restart(p, s, nm, (uint64_t)n0);
}

int stream_check_push(const StreamState &s, const StreamNames &nm, int64_t n) {
  // (an enqueue passes through here: a message is built only when it is needed)
  if (n < 1 || n > kStreamMaxPush) return fail(ZFFT_EINVAL, std::string(nm.who) + " push: " + nm.arg + " in [0, 2^31 - 1]");
  if (s.n + (uint64_t)n > kStreamMaxCount)
    return fail(ZFFT_EINVAL, std::string(nm.who) + " push: the " + nm.unit + " count would pass 2^62");
  return ZFFT_OK;
}

int stream_commit(zfft_plan *p, StreamState &s, int64_t n, hipStream_t st) {
  s.n += (uint64_t)n;
  s.par ^= 1;
  return done_on(p, st);
}

int stream_host_push(zfft_plan *p, StreamState &s, const StreamNames &nm, const void *in, size_t copy_bytes, void *out,
                     size_t out_bytes, const std::function<int(const void *d_in, void *d_out)> &body) {
  const std::string who = nm.who;
  if (!in || (out_bytes > 0 && !out)) return fail(ZFFT_EINVAL, who + " push: null host pointer");
  const size_t in_bytes = (copy_bytes + 15) & ~(size_t)15;
  int rc = grow(p, s.stage, in_bytes + out_bytes, (who + " staging").c_str());
  if (!rc) rc = use_stream(p, p->stream);  // the staging may still be read by the previous call
  if (rc) return rc;
  char *d = s.stage.as<char>();
  hipError_t e = hipMemcpyAsync(d, in, copy_bytes, hipMemcpyHostToDevice, p->stream);
  if (e != hipSuccess) return hip_fail(e, "H2D samples");
  rc = body(d, d + in_bytes);
  if (rc) return rc;
  e = out_bytes ? hipMemcpyAsync(out, d + in_bytes, out_bytes, hipMemcpyDeviceToHost, p->stream) : hipSuccess;
  return sync_read(p, e, (who + " push").c_str());
}

}  // namespace zfft
