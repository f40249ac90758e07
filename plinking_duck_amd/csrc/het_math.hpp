// het_math.hpp -- the per-variant expected homozygosity of pgh_het and its fixed-point form (host only; DESIGN.md
// section 3.15).
//
//   p = (het + 2 alt) / (2 called), or the caller's frequency        q = 1 - p        u = (2 p) q
//   with the small-sample correction   r = (2 called) / (2 called - 1)   u = u r
//   e = 1 - u                                                         (0 <= e <= 1)
//
// A variant is skipped when called == 0, or when p is not finite, p <= 0 or p >= 1.
// One IEEE operation per statement, as grm_math.hpp; here a product does feed a subtraction (e = 1 - u), so
// contraction into a fused multiply-add is switched off for the function: the result is the same on every host.
//
//   L = the smallest integer with 2^L >= max(n_var, 1)      k = 62 - L      q_v = llrint(e_v 2^k)
// so a sum of at most n_var such terms is an int64 that cannot pass 2^62.
#pragma once

#include "grm_math.hpp"

#include <cmath>
#include <cstdint>

namespace pgh {

// k of a call over n_var variants (the caller's count, also inside a shard group)
inline uint32_t HetScale(uint32_t n_var) {
	uint32_t l = 0;
	while ((1ull << l) < n_var) {
		l++;
	}
	return 62u - l;
}

// false: the variant is skipped and *e is left alone.  freq: NaN takes p from the counts.
inline bool HetExpected(uint32_t het, uint32_t alt, uint32_t called, double freq, bool small_sample, double *e) {
#pragma clang fp contract(off)
	if (called == 0) {
		return false;
	}
	const double p = std::isnan(freq) ? GrmFreq(het, alt, called) : freq;
	if (!(std::isfinite(p) && p > 0.0 && p < 1.0)) {
		return false;
	}
	const double q = 1.0 - p;
	const double tp = 2.0 * p;
	double u = tp * q;
	if (small_sample) {
		const double n2 = static_cast<double>(2ull * called); // exact: below 2^53
		const double n2m1 = static_cast<double>(2ull * called - 1ull);
		const double r = n2 / n2m1;
		u = u * r;
	}
	*e = 1.0 - u;
	return true;
}

// q_v of e under the scale k: e 2^k is exact (a power of two), llrint rounds it once, half to even
inline int64_t HetFixed(double e, uint32_t k) {
	return static_cast<int64_t>(std::llrint(std::ldexp(e, static_cast<int>(k))));
}

} // namespace pgh
