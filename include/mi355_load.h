/* mi355_load.h — C ABI of the Matrix Market ingest (libmi355load.so; host code only, no GPU).
 *
 * The reference's only input path is argv[1] -> LoadCoo -> ToCsr (main.cu:32-39, include/load.hpp:268-474): a
 * Matrix Market coordinate file becomes host CSR arrays that the harness uploads (main.cu:48-74).  The loader behind
 * these entry points is spmv-samples_amd/host/load.hpp — the same results entry for entry (1-based -> 0-based,
 * pattern -> 1.0, `symmetric` expanded entry-then-mirror in file order with the diagonal once, CSR by a stable
 * counting sort on the row, so file order survives inside a row and duplicates are kept), parsed in parallel from an
 * mmap.  The C++ harness (host/main.cpp) includes load.hpp directly; this ABI is for callers that are not C++ —
 * bench.py --mtx binds it with ctypes.
 *
 * Errors: the reference exits or throws (load.hpp:278-306, :324-360); here every failure is a status and a message.
 */
#ifndef MI355_LOAD_H
#define MI355_LOAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    MI355_LOAD_OK = 0,
    MI355_LOAD_EINVAL = 1,   /* null pointer / unknown type enum                                              */
    MI355_LOAD_EFILE = 2,    /* cannot open, not a Matrix Market coordinate file, unsupported field / symmetry */
    MI355_LOAD_EPARSE = 3,   /* short or malformed entry, zero-based index, index beyond the declared size     */
    MI355_LOAD_ERANGE = 4    /* rows / columns / entries do not fit index_t / offset_t                         */
};

typedef struct mi355_csr_host mi355_csr_host;

/* off_type: 0 = int32 offsets, 1 = int64 (MI355_OFF_*); val_type: 0 = float, 1 = double (MI355_VAL_*); index_t is
 * int32 (main.cu:15).  *out owns the arrays until mi355_csr_host_free.                                           */
int mi355_load_mtx(const char* path, int off_type, int val_type, mi355_csr_host** out);
int mi355_csr_host_dims(const mi355_csr_host* csr, int64_t* n_rows, int64_t* n_cols, int64_t* nnz);
/* the arrays themselves (host memory, valid until free): Ap has n_rows + 1 offsets of the loaded width             */
const void* mi355_csr_host_Ap(const mi355_csr_host* csr);
const int32_t* mi355_csr_host_Aj(const mi355_csr_host* csr);
const void* mi355_csr_host_Ax(const mi355_csr_host* csr);
void mi355_csr_host_free(mi355_csr_host* csr);

/* The COO that LoadCoo produces, before ToCsr (main.cu:32-39 runs the two in a row): entries in file order, 0-based,
 * `symmetric` expanded entry-then-mirror with the diagonal once, pattern values 1.0 — for callers that build the CSR
 * elsewhere (mi355_spmv_coo_to_csr in include/mi355_spmv.h, on the device).  Same types and error codes as
 * mi355_load_mtx: off_type only decides which sizes fit.  *out owns the arrays until mi355_load_coo_free.          */
typedef struct mi355_coo_host mi355_coo_host;
int mi355_load_mtx_coo(const char* path, int off_type, int val_type, mi355_coo_host** out);
int mi355_load_coo_dims(const mi355_coo_host* coo, int64_t* n_rows, int64_t* n_cols, int64_t* nnz);
/* nnz row and column indices (int32) and values (float or double, as loaded): host memory, valid until free        */
const int32_t* mi355_load_coo_rows(const mi355_coo_host* coo);
const int32_t* mi355_load_coo_cols(const mi355_coo_host* coo);
const void* mi355_load_coo_vals(const mi355_coo_host* coo);
void mi355_load_coo_free(mi355_coo_host* coo);

/* The file AS STORED, before LoadCoo's expansion: entries in file order, 0-based, pattern values 1.0, a `symmetric`
 * file's entries NOT mirrored — what mi355_spmv_coo_to_csr_symmetric (include/mi355_spmv.h) takes, so that only the
 * stored half crosses the bus.  The handle is a mi355_coo_host (dims: nnz = the stored entries; rows / cols / vals
 * and free as above).  *symmetric = 1 exactly when the banner says `symmetric`; *nnz_expanded = the entries
 * mi355_load_mtx_coo would return: nnz + the off-diagonal entries for a symmetric file, nnz otherwise
 * (skew-symmetric and hermitian files are not expanded, as in LoadCoo).  Same types, checks and error codes as
 * mi355_load_mtx_coo (a symmetric file's indices must fit both dimensions).                                          */
int mi355_load_mtx_stored(const char* path, int off_type, int val_type, mi355_coo_host** out, int* symmetric,
                          int64_t* nnz_expanded);

/* Message of the last failing call on this thread ("" if none).                                                    */
const char* mi355_load_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MI355_LOAD_H */
