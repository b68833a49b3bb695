// host_tocsr.cpp — the product's host ToCsr (spmv-samples_amd/host/load.hpp, the reference's include/load.hpp:420-474
// restated) behind one C call, for scripts/coo_csr_timing.py: it times the COO -> CSR step alone, on arrays the caller
// already holds, and hands back the CSR so that the device result can be compared with it.
//   g++ -std=c++17 -O2 -fPIC -shared -o libhosttocsr.so scripts/host_tocsr.cpp -lpthread
#include <algorithm>
#include <chrono>
#include <cstdint>

#define MI355_LOAD_NO_EXIT 1
#include "../spmv-samples_amd/host/load.hpp"

template <typename off_t, typename val_t>
static double run(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t* rows, const int32_t* cols,
                  const void* vals, void* Ap, int32_t* Aj, void* Ax) {
    coo_t<int, off_t, val_t> coo(n_rows, n_cols, off_t(nnz));
    std::copy(rows, rows + nnz, coo.row_indices.begin());
    std::copy(cols, cols + nnz, coo.column_indices.begin());
    std::copy(static_cast<const val_t*>(vals), static_cast<const val_t*>(vals) + nnz, coo.nonzero_values.begin());
    const auto t0 = std::chrono::steady_clock::now();
    const csr_t<int, off_t, val_t> csr = ToCsr(coo);
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::copy(csr.row_offsets.begin(), csr.row_offsets.end(), static_cast<off_t*>(Ap));
    std::copy(csr.column_indices.begin(), csr.column_indices.end(), Aj);
    std::copy(csr.nonzero_values.begin(), csr.nonzero_values.end(), static_cast<val_t*>(Ax));
    return seconds;
}

// off64 / val64: 64-bit offsets / double values.  Returns the seconds ToCsr took.
extern "C" double host_tocsr(int off64, int val64, int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t* rows,
                             const int32_t* cols, const void* vals, void* Ap, int32_t* Aj, void* Ax) {
    if (off64)
        return val64 ? run<long long, double>(n_rows, n_cols, nnz, rows, cols, vals, Ap, Aj, Ax)
                     : run<long long, float>(n_rows, n_cols, nnz, rows, cols, vals, Ap, Aj, Ax);
    return val64 ? run<int, double>(n_rows, n_cols, nnz, rows, cols, vals, Ap, Aj, Ax)
                 : run<int, float>(n_rows, n_cols, nnz, rows, cols, vals, Ap, Aj, Ax);
}
