// The gain rule of a stream delivered at a target loudness, written once: for
// stream_loudness_gain_kernel (stream_loudness.h) and for the one-utterance stream, whose conversion runs on the host.
#pragma once
#include <cmath>
#include "../pe_rt.h"
#include "params.h"

namespace pe {

// The rule of one chunk with n > 0 samples, written once for the gain kernel and for the
// one-utterance stream's host conversion. In: the running loudness L of the prefix (`ok`: measurable, `is_short`), the
// setting {T, C, prior (NaN: none)}, the running peak r' with this chunk in it, the previous end-of-chunk gain G, the
// stream's last used loudness `lu` (NaN: none yet) and `first`. Out: g0, g1, the flags, and `lu` moved on.
// lim (the look-ahead limiter on streams): the cap only marks -- g1 stays the target's gain, LIMITED | SHAPED
// where the cap is the smaller, and g0 is the previous gain uncut; stream_limiter_kernel holds the ceiling sample by sample.
struct SlRule { float g0, g1; int flags; };
__host__ __device__ __forceinline__ SlRule sl_rule(bool ok, bool is_short, double L, float T, float C, float prior, float rp, float G, bool first, float& lu,
                                                   bool lim = false) {
  SlRule o;
  o.flags = (is_short ? LOUD_SHORT : 0) | (ok ? 0 : LOUD_UNMEASURABLE);
  const bool has_prior = prior == prior;
  double Lu = 0.0;
  bool have = false;
  if (ok && !(is_short && has_prior)) { Lu = L; have = true; }
  else if (has_prior) { Lu = (double)prior; have = true; o.flags |= LOUD_PRIOR; }
  else if (lu == lu) { Lu = (double)lu; have = true; }
  if (have) lu = (float)Lu;
  const double a = have ? exp(((double)T - Lu) * 0.11512925464970228) : 1.0;      // 10^(x / 20) = e^(x ln 10 / 20)
  float cap = __builtin_inff();
  if (rp > 0.f) {
    const double lim = 32767.0 * (double)C;
    cap = (float)(lim / (double)rp);
    // (the rounding to f32 must not lift the running peak over the ceiling)
    if ((double)cap * (double)rp > lim) {
      unsigned u;
      __builtin_memcpy(&u, &cap, 4);
      --u;
      __builtin_memcpy(&cap, &u, 4);
    }
  }
  const float want = (float)(32767.0 * a);
  o.g1 = want;
  if (cap < want) {
    o.flags |= LOUD_LIMITED;
    if (lim) o.flags |= LOUD_SHAPED;
    else o.g1 = cap;
  }
  o.g0 = first ? o.g1 : (lim || G < cap ? G : cap);
  return o;
}

}  // namespace pe
