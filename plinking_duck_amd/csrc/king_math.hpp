// king_math.hpp -- the KING-robust kinship formula, shared by pgh_king_kinship (host) and the device filter of
// pgh_king_table (king.hip), so that a table row's KINSHIP is this function of the row's own counts bit for bit.
//
//   min_het = HETHET + min(HET1HOM2, HET2HOM1)
//   KINSHIP = 0.5 - (4 IBS0 + HET1HOM2 + HET2HOM1) / (4 min_het)        NaN when min_het == 0
//
// Integer sums first (exact in 64 bits: every count is below 2^32), one conversion each (exact: both sums are below
// 2^53), one division, one subtraction.  There is no multiply next to an add, so nothing can be contracted into a
// fused multiply-add, and IEEE division and subtraction are correctly rounded on the host and on the device.
#pragma once

#include <cstdint>
#include <limits>

#if defined(__HIPCC__)
#define PGH_KING_HD __host__ __device__
#else
#define PGH_KING_HD
#endif

namespace pgh {

PGH_KING_HD inline double KingKinship(uint32_t hethet, uint32_t ibs0, uint32_t het1hom2, uint32_t het2hom1) {
	const uint64_t min_het = static_cast<uint64_t>(hethet) + (het1hom2 < het2hom1 ? het1hom2 : het2hom1);
	if (min_het == 0) {
		return std::numeric_limits<double>::quiet_NaN();
	}
	const uint64_t num = 4ull * ibs0 + het1hom2 + het2hom1;
	const double n = static_cast<double>(num);
	const double d = static_cast<double>(4ull * min_het);
	const double q = n / d;
	return 0.5 - q;
}

} // namespace pgh
