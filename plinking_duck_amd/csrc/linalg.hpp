// linalg.hpp -- small dense host linear algebra for plink_pca's two thin SVDs
// (the reference calls Eigen::BDCSVD on the host, src/plink_pca.cpp:683-724;
// Eigen is not in this image).
#pragma once

#include <cstddef>
#include <vector>

namespace pgh {

// Thin SVD of the row-major m x n matrix a (m >= n): on return a holds U (m x n,
// orthonormal columns, same storage) and s the singular values in descending
// order.  Householder QR, then one-sided Jacobi on the n x n factor.
void ThinSvdInPlace(double *a, size_t m, size_t n, std::vector<double> &s);

// Eigen-decomposition of the symmetric n x n matrix g (row-major): eigenvalues in
// descending order, eigenvectors as the columns of v (n x n, row-major).  Cyclic Jacobi.
void SymmetricEigen(const std::vector<double> &g, size_t n, std::vector<double> &eigenvalues,
                    std::vector<double> &v);

// The eigenvalues alone of the symmetric n x n matrix a (row-major), in descending order: Householder
// tridiagonalisation and implicit QL, about 4/3 n^3 flops.  Returns false when the QL iteration did not converge and
// the values come from SymmetricEigen instead, or when an entry is not finite (out is then all NaN).  Shared with pgh_skat_sparse (one matrix per variant set).
bool SymmetricEigenvalues(const double *a, size_t n, double *out);

} // namespace pgh
