// The guard bands of the rk_debug_* entry points (debug_calls.inc): ONE owner of their arithmetic and of the rule an
// rk_debug_rows_out must keep.  Every output of a debug call is a device allocation [band | interior | band]: the bands hold the
// byte RK_DEBUG_SENTINEL before the launch and the whole allocation is copied back behind it.  Plain C++17, no HIP: a CPU program
// includes this header too (tests/test_debug_bands_host.py).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/rk_engine.h"

struct BandSpan {
  size_t bytes, band;                                      // the interior and ONE band, in bytes
  size_t all() const { return bytes + 2 * band; }          // the whole allocation
  size_t interior() const { return band; }                 // where the interior starts
};
// the row form: bands of band_rows rows of ld elements of elt bytes around an interior of n elements
inline BandSpan band_rows_span(size_t n, size_t band_rows, size_t ld, size_t elt) { return BandSpan{n * elt, band_rows * ld * elt}; }

// an rk_debug_rows_out against the `need` bytes its call addresses: interior and all present; a band of at least 64 bytes, a
// multiple of 16, at most 2^26; then the caller's comparison - AT_LEAST (rk_debug_rows: need <= bytes <= 2^31, the interior may
// be larger than what the launch touches) or EXACT (rk_debug_draft_steps: the kernels take the arrays' lengths from the state)
enum BandNeed { BAND_AT_LEAST, BAND_EXACT };
inline bool band_out_ok(const rk_debug_rows_out& b, int64_t need, BandNeed how) {
  if (!b.interior || !b.all || b.band < 64 || b.band % 16 || b.band > (1 << 26)) return false;
  return how == BAND_EXACT ? need == b.bytes : (need <= b.bytes && b.bytes <= ((int64_t)1 << 31));
}
