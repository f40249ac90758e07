// The rules of variant ranges and variant lists (plinking_duck_amd/csrc/variant_rows.hpp) on the host alone, over
// the resident range [37, 318) of tests/variant_shapes.py.  Built and run by tests/test_variant_rows_host.py under
// AddressSanitizer + UBSan; exit status 0 and "variant rows ok" when every check holds.
#include "variant_rows.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

namespace {

constexpr uint32_t kB = 37, kE = 318;
const std::string kOutside = "outside the resident range";
const std::string kIncreasing = "the variant list must be strictly increasing";

int failures = 0;

void Check(bool ok, const char *what, int line) {
	if (!ok) {
		std::fprintf(stderr, "line %d: %s\n", line, what);
		failures++;
	}
}
#define CHECK(cond) Check((cond), #cond, __LINE__)

bool IsOutside(const std::string &err) {
	return err.find(kOutside) != std::string::npos;
}

struct Resolved {
	std::string err;
	uint32_t first = 0xdeadbeefu;
	std::vector<uint32_t> local;
};

Resolved Range(uint32_t variant_begin, uint32_t n, uint32_t flags = 0) {
	Resolved r;
	r.local.assign(3, 7u); // stale content must not survive
	r.err = pgh::ResolveVariantRows(kB, kE, variant_begin, n, nullptr, flags, r.first, r.local);
	return r;
}

Resolved List(const std::vector<uint32_t> &vidx, uint32_t flags = 0) {
	Resolved r;
	// an exact-size heap copy (null where empty), so that a read past the list is the sanitizer's to find
	uint32_t *copy = vidx.empty() ? nullptr : static_cast<uint32_t *>(std::malloc(sizeof(uint32_t) * vidx.size()));
	if (copy) {
		std::memcpy(copy, vidx.data(), sizeof(uint32_t) * vidx.size());
	}
	r.err = pgh::ResolveVariantRows(kB, kE, 0, static_cast<uint32_t>(vidx.size()), copy,
	                                flags | pgh::kVariantRowsListOnly, r.first, r.local);
	// the validate-only form agrees with the translating one
	const std::string only = pgh::VariantListError(kB, kE, static_cast<uint32_t>(vidx.size()), copy,
	                                               (flags & pgh::kVariantRowsIncreasing) != 0);
	CHECK(only == r.err);
	std::free(copy);
	return r;
}

void PassesAsList(const std::vector<uint32_t> &vidx, uint32_t flags = 0) {
	const Resolved r = List(vidx, flags);
	CHECK(r.err.empty());
	CHECK(r.first == 0);
	CHECK(r.local.size() == vidx.size());
	for (size_t i = 0; i < vidx.size() && i < r.local.size(); i++) {
		CHECK(r.local[i] == vidx[i] - kB);
	}
}

void RangeForm() {
	for (const auto &[vb, n] : {std::pair<uint32_t, uint32_t> {37, 0}, {37, 281}, {318, 0}, {100, 57}}) {
		const Resolved plain = Range(vb, n);
		CHECK(plain.err.empty());
		CHECK(plain.first == vb - kB);
		CHECK(plain.local.empty()); // no list unless asked for: the kernels take (first, null)
		const Resolved expanded = Range(vb, n, pgh::kVariantRowsExpand);
		CHECK(expanded.err.empty());
		CHECK(expanded.first == vb - kB);
		CHECK(expanded.local.size() == n);
		for (uint32_t i = 0; i < expanded.local.size(); i++) {
			CHECK(expanded.local[i] == expanded.first + i);
		}
	}
	// (0xFFFFFFF0, 0x20): the 32-bit sum wraps to 0x10
	for (const auto &[vb, n] : {std::pair<uint32_t, uint32_t> {36, 1}, {318, 1}, {300, 19}, {300, 0xFFFFFFFFu},
	                            {0xFFFFFFF0u, 0x20}}) {
		for (const uint32_t flags : {0u, static_cast<uint32_t>(pgh::kVariantRowsExpand)}) {
			const Resolved r = Range(vb, n, flags);
			CHECK(IsOutside(r.err));
			CHECK(r.local.empty());
		}
	}
	// the (begin, end) form that the range-only entry points check
	CHECK(pgh::VariantRangeError(kB, kE, 37, 318).empty());
	CHECK(pgh::VariantRangeError(kB, kE, 200, 200).empty());
	CHECK(IsOutside(pgh::VariantRangeError(kB, kE, 201, 200)));
	CHECK(IsOutside(pgh::VariantRangeError(kB, kE, 36, 318)));
	CHECK(IsOutside(pgh::VariantRangeError(kB, kE, 37, 319)));
}

void ListForm() {
	std::vector<uint32_t> all(kE - kB);
	std::iota(all.begin(), all.end(), kB);
	std::vector<uint32_t> reversed(all.rbegin(), all.rend());
	std::vector<uint32_t> shuffled(all.size());
	for (size_t i = 0; i < all.size(); i++) {
		shuffled[i] = all[i * 100 % all.size()]; // 100 and 281 are coprime: a permutation
	}
	PassesAsList({37});
	PassesAsList({317});
	PassesAsList(all);
	PassesAsList(reversed);
	PassesAsList(shuffled);
	PassesAsList({200, 200, 37, 200, 317, 317});
	PassesAsList({});
	CHECK(IsOutside(List({36}).err));
	CHECK(IsOutside(List({318}).err));
	CHECK(IsOutside(List({0xFFFFFFFFu}).err));
	std::vector<uint32_t> one_bad = all;
	one_bad[one_bad.size() / 2] = 318;
	CHECK(IsOutside(List(one_bad).err));
	one_bad[one_bad.size() / 2] = 36;
	CHECK(IsOutside(List(one_bad).err));
	// the entry-by-entry form of the pair calls
	CHECK(pgh::VariantInside(kB, kE, 37) && pgh::VariantInside(kB, kE, 317));
	CHECK(!pgh::VariantInside(kB, kE, 36) && !pgh::VariantInside(kB, kE, 318) && !pgh::VariantInside(kB, kE, 0));
	CHECK(pgh::VariantOutsideError(kB, kE, 5, 318) == List({40, 41, 42, 43, 44, 318, 45}).err);
	// a null list is the range form unless the entry point has none
	uint32_t first = 0;
	std::vector<uint32_t> local;
	CHECK(pgh::VariantListError(kB, kE, 0, nullptr, false).empty());
	CHECK(pgh::ResolveVariantRows(kB, kE, 0, 0, nullptr, pgh::kVariantRowsListOnly, first, local).empty());
	CHECK(IsOutside(pgh::ResolveVariantRows(kB, kE, 0, 0, nullptr, 0, first, local)));
}

void IncreasingRule() {
	const uint32_t inc = pgh::kVariantRowsIncreasing;
	PassesAsList({40, 41}, inc);
	PassesAsList({37, 100, 317}, inc);
	CHECK(List({40, 40}, inc).err == kIncreasing);
	CHECK(List({41, 40}, inc).err == kIncreasing);
	CHECK(List({50, 40, 400}, inc).err == kIncreasing); // the earlier entry wins
	CHECK(IsOutside(List({50, 400, 40}, inc).err));
	CHECK(IsOutside(List({50, 36}, inc).err)); // one entry breaks both rules: "outside" is tested first
	// without the flag the ones in range pass
	PassesAsList({40, 40});
	PassesAsList({41, 40});
	CHECK(IsOutside(List({50, 40, 400}).err));
	CHECK(IsOutside(List({50, 400, 40}).err));
	CHECK(kIncreasing == pgh::kVariantListNotIncreasing);
}

} // namespace

int main() {
	RangeForm();
	ListForm();
	IncreasingRule();
	if (failures) {
		std::fprintf(stderr, "%d checks failed\n", failures);
		return 1;
	}
	std::puts("variant rows ok");
	return 0;
}
