// ld_math.hpp -- the "r2 exceeds the threshold" test and the minor-allele order of pgh_ld_prune, and the r2 term of
// pgh_ld_scores, shared by pgh_ld_exceeds / pgh_ld_r2 (host), the host pruning loop (api_ldband.cpp) and the device
// epilogues of k_ld_band (ldband.hip), so that a pair's bit, and a pair's term, is this function of the pair's own six
// sums on the host and on the device alike.
//
//   num = n sum_ab - sum_a sum_b      va = n sum_a2 - sum_a^2      vb = n sum_b2 - sum_b^2        (int64)
//   n < 2, va <= 0 or vb <= 0: never exceeds (a variant that is monomorphic over the pair's samples has no r2)
//   r2 = ((double)num * (double)num) / ((double)va * (double)vb)      exceeds iff r2 > threshold
//
// The int64 terms are exact for the sums the library produces: n <= 2^29 - 1 samples, so sum_a, sum_b <= 2^30,
// sum_ab, sum_a2, sum_b2 <= 2^31 and every product is below 2^61.  After that there are three conversions, two
// multiplications and one division, each correctly rounded, and no addition next to a product: nothing can be
// contracted into a fused multiply-add, so the host, the device and numpy give the same bits.
// This is NOT plink_ld's arithmetic (the reference's mean-based doubles on the same sums); plink_ld keeps that.
//
// LdR2Term (pgh_ld_scores) is the same r2, returned instead of compared, and with kLdScoreUnbiased
//   term = r2 - (1.0 - r2) / (double)(n - 2)        (needs n >= 3; n - 2 converts exactly)
// as one subtraction, one division and one subtraction in statements of their own: again no product next to a sum.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PGH_LD_HD __host__ __device__
#else
#define PGH_LD_HD
#endif

namespace pgh {

constexpr uint32_t kLdBandMaxSamples = (1u << 29) - 1; // 4 (2^29 - 1) < 2^31: an int32 accumulator holds any sum
constexpr uint32_t kLdScoreUnbiased = 1u;              // PGH_LDSCORE_UNBIASED

PGH_LD_HD inline bool LdExceeds(uint32_t n, uint32_t sum_a, uint32_t sum_b, uint32_t sum_ab, uint32_t sum_a2,
                                uint32_t sum_b2, double threshold) {
	if (n < 2) {
		return false;
	}
	const int64_t nn = n, sa = sum_a, sb = sum_b;
	const int64_t num = nn * static_cast<int64_t>(sum_ab) - sa * sb;
	const int64_t va = nn * static_cast<int64_t>(sum_a2) - sa * sa;
	const int64_t vb = nn * static_cast<int64_t>(sum_b2) - sb * sb;
	if (va <= 0 || vb <= 0) {
		return false;
	}
	const double dn = static_cast<double>(num);
	const double top = dn * dn;
	const double bottom = static_cast<double>(va) * static_cast<double>(vb);
	const double r2 = top / bottom;
	return r2 > threshold;
}

// The pair's term of an LD score; false (and *term untouched) when the pair has no r2: n < 2 (n < 3 with
// kLdScoreUnbiased), va <= 0 or vb <= 0.
PGH_LD_HD inline bool LdR2Term(uint32_t n, uint32_t sum_a, uint32_t sum_b, uint32_t sum_ab, uint32_t sum_a2,
                               uint32_t sum_b2, uint32_t flags, double *term) {
	const bool unbiased = (flags & kLdScoreUnbiased) != 0;
	if (n < (unbiased ? 3u : 2u)) {
		return false;
	}
	const int64_t nn = n, sa = sum_a, sb = sum_b;
	const int64_t num = nn * static_cast<int64_t>(sum_ab) - sa * sb;
	const int64_t va = nn * static_cast<int64_t>(sum_a2) - sa * sa;
	const int64_t vb = nn * static_cast<int64_t>(sum_b2) - sb * sb;
	if (va <= 0 || vb <= 0) {
		return false;
	}
	const double dn = static_cast<double>(num);
	const double top = dn * dn;
	const double dva = static_cast<double>(va);
	const double dvb = static_cast<double>(vb);
	const double bottom = dva * dvb;
	const double r2 = top / bottom;
	if (!unbiased) {
		*term = r2;
		return true;
	}
	const double rest = 1.0 - r2;
	const double dof = static_cast<double>(n - 2u);
	const double adj = rest / dof;
	*term = r2 - adj;
	return true;
}

// Per variant over the output samples: alt = het + 2 hom_alt, obs = 2 called, mc = min(alt, obs - alt).
// k has the lower minor-allele frequency than u iff mc_k obs_u < mc_u obs_k (uint64: both factors are at most 2^30);
// a variant without a call (obs = 0) compares as equal to everything.
inline bool LdLowerMaf(uint32_t mc_k, uint32_t obs_k, uint32_t mc_u, uint32_t obs_u) {
	return static_cast<uint64_t>(mc_k) * obs_u < static_cast<uint64_t>(mc_u) * obs_k;
}

} // namespace pgh
