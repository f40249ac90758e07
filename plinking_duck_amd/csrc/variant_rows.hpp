// variant_rows.hpp -- the rules of pgenhip.h's section "variant ranges and variant lists", once: a caller's GLOBAL
// variant range or list against a resident range [b, e), turned into rows of that range (row = index - b).
// Plain C++17 with no HIP and no handle types, so that a stand-alone host program can test it
// (tests/host/variant_rows_main.cpp); api_internal.hpp:VariantRows puts the device list on top.
// Every function returns the text of its refusal, empty when there is none.
#pragma once

#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

namespace pgh {

constexpr const char *kVariantListNotIncreasing = "the variant list must be strictly increasing";

enum : uint32_t {
	kVariantRowsExpand = 1u,     // a range is written out as a list of rows as well
	kVariantRowsIncreasing = 2u, // a list must be strictly increasing
	kVariantRowsListOnly = 4u,   // the entry point has no range form: vidx is its list, null where that is empty
};

//! [begin, end) must be ordered and inside [b, e).  64-bit ends: variant_begin + n is passed as it is, never wrapped.
inline std::string VariantRangeError(uint32_t b, uint32_t e, uint64_t begin, uint64_t end) {
	if (begin <= end && begin >= b && end <= e) {
		return {};
	}
	char msg[200];
	std::snprintf(msg, sizeof msg, "variant range [%llu, %llu) is outside the resident range [%u, %u)",
	              static_cast<unsigned long long>(begin), static_cast<unsigned long long>(end), b, e);
	return msg;
}

//! One entry of a list against [b, e), for the pair calls, which check while they walk their two lists once ...
inline bool VariantInside(uint32_t b, uint32_t e, uint32_t v) {
	return v >= b && v < e;
}

//! ... and the refusal of list entry i, v, that is not.
inline std::string VariantOutsideError(uint32_t b, uint32_t e, uint32_t i, uint32_t v) {
	char msg[200];
	std::snprintf(msg, sizeof msg, "variant index %u (list entry %u) is outside the resident range [%u, %u)", v, i, b, e);
	return msg;
}

//! Every vidx[0..n) must lie in [b, e) and, with `increasing`, exceed the entry before it; the first entry that breaks
//! a rule is the one refused, "outside" before "not increasing".  local (unless null): local[i] = vidx[i] - b.
inline std::string VariantListError(uint32_t b, uint32_t e, uint32_t n, const uint32_t *vidx, bool increasing,
                                    uint32_t *local = nullptr) {
	for (uint32_t i = 0; i < n; i++) {
		if (!VariantInside(b, e, vidx[i])) {
			return VariantOutsideError(b, e, i, vidx[i]);
		}
		if (increasing && i && vidx[i] <= vidx[i - 1]) {
			return kVariantListNotIncreasing;
		}
		if (local) {
			local[i] = vidx[i] - b;
		}
	}
	return {};
}

//! The two forms of (variant_begin, n, vidx).  vidx == NULL: the range; first = its first row, and local = first + i
//! with kVariantRowsExpand, else empty.  vidx != NULL: the list; first = 0 and local = its rows.
inline std::string ResolveVariantRows(uint32_t b, uint32_t e, uint32_t variant_begin, uint32_t n, const uint32_t *vidx,
                                      uint32_t flags, uint32_t &first, std::vector<uint32_t> &local) {
	first = 0;
	local.clear();
	if (vidx || (flags & kVariantRowsListOnly)) {
		local.resize(n);
		return VariantListError(b, e, n, vidx, (flags & kVariantRowsIncreasing) != 0, local.data());
	}
	std::string err = VariantRangeError(b, e, variant_begin, static_cast<uint64_t>(variant_begin) + n);
	if (err.empty()) {
		first = variant_begin - b;
		if (flags & kVariantRowsExpand) {
			local.resize(n);
			std::iota(local.begin(), local.end(), first);
		}
	}
	return err;
}

} // namespace pgh
