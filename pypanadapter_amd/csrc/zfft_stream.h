// zfft_stream.h -- the host path the producers on a sample stream share (zfft_tap.cpp,
// zfft_chan.cpp, zfft_demod.cpp, zfft_resamp.cpp, zfft_level.cpp): the count and its limits, the two
// alternating carries and the staging of a host push.  The counting rule itself is pure
// (zfft_stream_plan.h).  Not part of the C-ABI.
#pragma once

#include <functional>

#include "zfft_plan.h"

namespace zfft {

// How a producer's messages name it, its push argument and the unit it counts: {"demod", "steps", "step"}.
struct StreamNames {
  const char *who, *arg, *unit;
};

// What every producer carries.  The count is the host's: pushes are in call order, so it is known
// when a push is enqueued.  A push reads the carry of parity `par` and writes the other.
struct StreamState {
  uint64_t n = 0;        // units given
  int par = 0;
  size_t carry_len = 0;  // float2 of one carry
  DevBuf carry, stage;   // the two carries; the device staging of the producer's own host push
  float2 *carry_in() const { return carry.as<float2>() + (size_t)par * carry_len; }
  float2 *carry_out() const { return carry.as<float2>() + (size_t)(par ^ 1) * carry_len; }
};

// Two carries of len float2 each (stream_restart zeroes them).
inline hipError_t stream_alloc(StreamState &s, size_t len) {
  s.carry_len = len;
  return s.carry.ensure(2 * len * sizeof(float2));
}
// The count to n0, the parity to 0 and both carries to zeros, in stream order on the plan's stream.
int stream_restart(zfft_plan *p, StreamState &s, const StreamNames &nm, uint64_t n0);
// The same for a caller's n0: ZFFT_EINVAL outside [0, 2^62].
int stream_reset(zfft_plan *p, StreamState &s, const StreamNames &nm, int64_t n0);
// A push of n units: 1 <= n <= 2^31 - 1 and a count that stays within 2^62, else ZFFT_EINVAL.
int stream_check_push(const StreamState &s, const StreamNames &nm, int64_t n);
// After a push of n units was enqueued on st: the count forward, the parity flipped, done_on.
int stream_commit(zfft_plan *p, StreamState &s, int64_t n, hipStream_t st);
// A synchronous push from host memory: copy_bytes of `in` into the producer's staging (the input
// rounded up to 16 bytes, then out_bytes), body(d_in, d_out) -- the producer's device push on
// p->stream -- and out_bytes back into `out`.  Every copy and launch of it goes on p->stream and
// it waits for them before it returns, so no later call finds the staging in use.
int stream_host_push(zfft_plan *p, StreamState &s, const StreamNames &nm, const void *in, size_t copy_bytes, void *out,
                     size_t out_bytes, const std::function<int(const void *d_in, void *d_out)> &body);

}  // namespace zfft
