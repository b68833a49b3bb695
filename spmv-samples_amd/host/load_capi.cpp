// load_capi.cpp — the extern "C" surface of include/mi355_load.h around host/load.hpp (LoadCoo + ToCsr, the
// reference's include/load.hpp:268-474 restated for speed): what bench.py --mtx and other non-C++ callers bind; and
// LoadCoo alone (mi355_load_mtx_coo) and the file as stored (mi355_load_mtx_stored), for callers that build the CSR on
// the device.
// The reference exits the process on a bad file (load.hpp:278-300); a library must not, so the loader runs with
// its exit-on-error switched to exceptions (MI355_LOAD_NO_EXIT) and everything becomes a status + message.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#define MI355_LOAD_NO_EXIT 1
#include "load.hpp"
#include "../../include/mi355_load.h"

struct mi355_csr_host {
    int off_type = 0, val_type = 0;
    csr_t<int, int, float> a;
    csr_t<int, int, double> b;
    csr_t<int, long long, float> c;
    csr_t<int, long long, double> d;
};

// LoadCoo's result before ToCsr: file order, `symmetric` expanded entry-then-mirror.  The offset type only decides
// which sizes fit (as for mi355_load_mtx); the values are float or double.
struct mi355_coo_host {
    int val_type = 0;
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    std::vector<int> rows, cols;
    std::vector<float> vf;
    std::vector<double> vd;
};

namespace {
thread_local char g_err[512] = "";
void set_err(const char* m) { std::snprintf(g_err, sizeof(g_err), "%s", m); }

template <typename off_t, typename val_t>
void take_coo(mi355_coo_host& into, coo_t<int, off_t, val_t>&& coo) {
    into.n_rows = coo.number_of_rows;
    into.n_cols = coo.number_of_columns;
    into.nnz = int64_t(coo.number_of_nonzeros);
    into.rows.swap(coo.row_indices);
    into.cols.swap(coo.column_indices);
    if constexpr (sizeof(val_t) == 8) into.vd.swap(coo.nonzero_values);
    else into.vf.swap(coo.nonzero_values);
}

// Runs one load step and turns the loader's exceptions into a status + message.
template <typename Step>
int guarded(Step&& step) {
    try {
        step();
        return MI355_LOAD_OK;
    } catch (const mm_detail::fatal_t& e) {
        set_err(e.what());
        return MI355_LOAD_EFILE;
    } catch (const exception_t& e) {
        set_err(e.what());
        return std::strstr(e.what(), "overflow") ? MI355_LOAD_ERANGE : MI355_LOAD_EPARSE;
    } catch (const std::bad_alloc&) {
        set_err("out of host memory");
        return MI355_LOAD_ERANGE;
    }
}

template <typename Csr>
int fill(Csr& into, const char* path) {
    using off_t = typename std::remove_reference<decltype(into.row_offsets[0])>::type;
    using val_t = typename std::remove_reference<decltype(into.nonzero_values[0])>::type;
    return guarded([&] { into = ToCsr(LoadCoo<int, off_t, val_t>(std::string(path))); });
}

template <typename off_t, typename val_t>
int fill_coo(mi355_coo_host& into, const char* path) {
    return guarded([&] { take_coo(into, LoadCoo<int, off_t, val_t>(std::string(path))); });
}

template <typename off_t, typename val_t>
int fill_stored(mi355_coo_host& into, const char* path, bool* symmetric, uint64_t* off_diagonal) {
    return guarded([&] { take_coo(into, LoadCooStored<int, off_t, val_t>(std::string(path), symmetric, off_diagonal)); });
}
}  // namespace

extern "C" {

int mi355_load_mtx(const char* path, int off_type, int val_type, mi355_csr_host** out) {
    g_err[0] = 0;
    if (!path || !out || (off_type != 0 && off_type != 1) || (val_type != 0 && val_type != 1)) {
        set_err("mi355_load_mtx: null pointer or unknown type");
        return MI355_LOAD_EINVAL;
    }
    *out = nullptr;
    mi355_csr_host* h = new (std::nothrow) mi355_csr_host();
    if (!h) { set_err("out of host memory"); return MI355_LOAD_ERANGE; }
    h->off_type = off_type;
    h->val_type = val_type;
    const int st = off_type == 0 ? (val_type == 0 ? fill(h->a, path) : fill(h->b, path))
                                 : (val_type == 0 ? fill(h->c, path) : fill(h->d, path));
    if (st != MI355_LOAD_OK) { delete h; return st; }
    *out = h;
    return MI355_LOAD_OK;
}

#define MI355_PICK(h, expr) ((h)->off_type == 0 ? ((h)->val_type == 0 ? (h)->a.expr : (h)->b.expr) \
                                                : ((h)->val_type == 0 ? (h)->c.expr : (h)->d.expr))

int mi355_csr_host_dims(const mi355_csr_host* h, int64_t* n_rows, int64_t* n_cols, int64_t* nnz) {
    if (!h || !n_rows || !n_cols || !nnz) { set_err("mi355_csr_host_dims: null pointer"); return MI355_LOAD_EINVAL; }
    *n_rows = int64_t(MI355_PICK(h, number_of_rows));
    *n_cols = int64_t(MI355_PICK(h, number_of_columns));
    *nnz = int64_t(MI355_PICK(h, number_of_nonzeros));
    return MI355_LOAD_OK;
}
const void* mi355_csr_host_Ap(const mi355_csr_host* h) {
    if (!h) return nullptr;
    return h->off_type == 0 ? (h->val_type == 0 ? static_cast<const void*>(h->a.row_offsets.data()) : h->b.row_offsets.data())
                            : (h->val_type == 0 ? static_cast<const void*>(h->c.row_offsets.data()) : h->d.row_offsets.data());
}
const int32_t* mi355_csr_host_Aj(const mi355_csr_host* h) {
    if (!h) return nullptr;
    return reinterpret_cast<const int32_t*>(MI355_PICK(h, column_indices.data()));
}
const void* mi355_csr_host_Ax(const mi355_csr_host* h) {
    if (!h) return nullptr;
    return h->off_type == 0 ? (h->val_type == 0 ? static_cast<const void*>(h->a.nonzero_values.data()) : h->b.nonzero_values.data())
                            : (h->val_type == 0 ? static_cast<const void*>(h->c.nonzero_values.data()) : h->d.nonzero_values.data());
}
void mi355_csr_host_free(mi355_csr_host* h) { delete h; }

int mi355_load_mtx_coo(const char* path, int off_type, int val_type, mi355_coo_host** out) {
    g_err[0] = 0;
    if (!path || !out || (off_type != 0 && off_type != 1) || (val_type != 0 && val_type != 1)) {
        set_err("mi355_load_mtx_coo: null pointer or unknown type");
        return MI355_LOAD_EINVAL;
    }
    *out = nullptr;
    mi355_coo_host* h = new (std::nothrow) mi355_coo_host();
    if (!h) { set_err("out of host memory"); return MI355_LOAD_ERANGE; }
    h->val_type = val_type;
    const int st = off_type == 0 ? (val_type == 0 ? fill_coo<int, float>(*h, path) : fill_coo<int, double>(*h, path))
                                 : (val_type == 0 ? fill_coo<long long, float>(*h, path)
                                                  : fill_coo<long long, double>(*h, path));
    if (st != MI355_LOAD_OK) { delete h; return st; }
    *out = h;
    return MI355_LOAD_OK;
}
int mi355_load_mtx_stored(const char* path, int off_type, int val_type, mi355_coo_host** out, int* symmetric,
                          int64_t* nnz_expanded) {
    g_err[0] = 0;
    if (!path || !out || !symmetric || !nnz_expanded || (off_type != 0 && off_type != 1) ||
        (val_type != 0 && val_type != 1)) {
        set_err("mi355_load_mtx_stored: null pointer or unknown type");
        return MI355_LOAD_EINVAL;
    }
    *out = nullptr;
    mi355_coo_host* h = new (std::nothrow) mi355_coo_host();
    if (!h) { set_err("out of host memory"); return MI355_LOAD_ERANGE; }
    h->val_type = val_type;
    bool sym = false;
    uint64_t off_diag = 0;
    const int st = off_type == 0 ? (val_type == 0 ? fill_stored<int, float>(*h, path, &sym, &off_diag)
                                                  : fill_stored<int, double>(*h, path, &sym, &off_diag))
                                 : (val_type == 0 ? fill_stored<long long, float>(*h, path, &sym, &off_diag)
                                                  : fill_stored<long long, double>(*h, path, &sym, &off_diag));
    if (st != MI355_LOAD_OK) { delete h; return st; }
    *out = h;
    *symmetric = sym ? 1 : 0;
    *nnz_expanded = h->nnz + int64_t(off_diag);
    return MI355_LOAD_OK;
}
int mi355_load_coo_dims(const mi355_coo_host* h, int64_t* n_rows, int64_t* n_cols, int64_t* nnz) {
    if (!h || !n_rows || !n_cols || !nnz) { set_err("mi355_load_coo_dims: null pointer"); return MI355_LOAD_EINVAL; }
    *n_rows = h->n_rows;
    *n_cols = h->n_cols;
    *nnz = h->nnz;
    return MI355_LOAD_OK;
}
const int32_t* mi355_load_coo_rows(const mi355_coo_host* h) { return h ? reinterpret_cast<const int32_t*>(h->rows.data()) : nullptr; }
const int32_t* mi355_load_coo_cols(const mi355_coo_host* h) { return h ? reinterpret_cast<const int32_t*>(h->cols.data()) : nullptr; }
const void* mi355_load_coo_vals(const mi355_coo_host* h) {
    if (!h) return nullptr;
    return h->val_type == 0 ? static_cast<const void*>(h->vf.data()) : static_cast<const void*>(h->vd.data());
}
void mi355_load_coo_free(mi355_coo_host* h) { delete h; }
const char* mi355_load_last_error(void) { return g_err; }

}  // extern "C"
