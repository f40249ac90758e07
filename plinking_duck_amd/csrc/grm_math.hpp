// grm_math.hpp -- the variance standardisation of pgh_grm (host only).
//
//   p = (het + 2 alt) / (2 called)          q = 1 - p          s = sqrt((2 p) q)
//   z[c] = (c - 2 p) / s   for the codes c = 0, 1, 2           (a missing call contributes 0)
//
// A variant is skipped when called == 0, or when p is not finite, p <= 0 or p >= 1.
// One IEEE operation per line and no multiply feeding an add (2 p is exact, so c - 2 p has one rounding whatever
// the compiler does with it): nothing here can be contracted into a fused multiply-add, and the result is the same
// on every host.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>

namespace pgh {

// p from the class counts over the output samples; NaN when nothing is called
inline double GrmFreq(uint32_t het, uint32_t alt, uint32_t called) {
	if (called == 0) {
		return std::numeric_limits<double>::quiet_NaN();
	}
	const double num = static_cast<double>(static_cast<uint64_t>(het) + 2ull * alt); // exact: below 2^53
	const double den = static_cast<double>(2ull * called);
	return num / den;
}

// false: the variant is skipped and z is left alone
inline bool GrmTable(double p, double z[3]) {
	if (!(std::isfinite(p) && p > 0.0 && p < 1.0)) {
		return false;
	}
	const double q = 1.0 - p;
	const double tp = 2.0 * p;
	const double var = tp * q;
	const double s = std::sqrt(var);
	const double d0 = 0.0 - tp, d1 = 1.0 - tp, d2 = 2.0 - tp;
	z[0] = d0 / s;
	z[1] = d1 / s;
	z[2] = d2 / s;
	return true;
}

} // namespace pgh
