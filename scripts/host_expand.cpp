// host_expand.cpp — the product's host expansion of a `symmetric` file's stored entries (spmv-samples_amd/host/load.hpp
// ExpandSymmetric, the reference's include/load.hpp:362-403 restated) behind one C call, for scripts/coo_sym_timing.py:
// it times the expansion loop alone, on arrays the caller already holds, and hands back the expanded COO so that the
// parent path (upload + mi355_spmv_coo_to_csr) and the host ToCsr (scripts/host_tocsr.cpp) can run on it.
//   g++ -std=c++17 -O2 -fPIC -shared -o libhostsym.so scripts/host_expand.cpp scripts/host_tocsr.cpp -lpthread
#include <algorithm>
#include <chrono>
#include <cstdint>

#define MI355_LOAD_NO_EXIT 1
#include "../spmv-samples_amd/host/load.hpp"

template <typename val_t>
static double run(int32_t n, int64_t nnz_stored, int64_t nnz_expanded, const int32_t* rows, const int32_t* cols,
                  const void* vals, int32_t* out_rows, int32_t* out_cols, void* out_vals) {
    coo_t<int, long long, val_t> coo(n, n, nnz_stored);
    std::copy(rows, rows + nnz_stored, coo.row_indices.begin());
    std::copy(cols, cols + nnz_stored, coo.column_indices.begin());
    std::copy(static_cast<const val_t*>(vals), static_cast<const val_t*>(vals) + nnz_stored, coo.nonzero_values.begin());
    const auto t0 = std::chrono::steady_clock::now();
    // as LoadCoo did before the count moved into the parse: one serial count, then the copy loop
    uint64_t off_diag = 0;
    for (int64_t i = 0; i < nnz_stored; ++i) off_diag += coo.row_indices[size_t(i)] != coo.column_indices[size_t(i)];
    ExpandSymmetric(coo, off_diag);
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (int64_t(coo.number_of_nonzeros) != nnz_expanded) return -1.0;
    std::copy(coo.row_indices.begin(), coo.row_indices.end(), out_rows);
    std::copy(coo.column_indices.begin(), coo.column_indices.end(), out_cols);
    std::copy(coo.nonzero_values.begin(), coo.nonzero_values.end(), static_cast<val_t*>(out_vals));
    return seconds;
}

// val64: double values.  Returns the seconds the count + expansion took (-1: nnz_expanded is not what it expands to).
extern "C" double host_expand(int val64, int32_t n, int64_t nnz_stored, int64_t nnz_expanded, const int32_t* rows,
                              const int32_t* cols, const void* vals, int32_t* out_rows, int32_t* out_cols,
                              void* out_vals) {
    return val64 ? run<double>(n, nnz_stored, nnz_expanded, rows, cols, vals, out_rows, out_cols, out_vals)
                 : run<float>(n, nnz_stored, nnz_expanded, rows, cols, vals, out_rows, out_cols, out_vals);
}
