// capi.hip — the extern "C" surface declared in include/mi355_spmv.h.
// Plan life cycle, argument checks, type dispatch.  No CPU compute path exists
// in this library: every entry point either launches HIP kernels or fails.

#include <algorithm>
#include <cstdarg>
#include <mutex>
#include <new>
#include <type_traits>

#include "common.hpp"

struct mi355_spmv_plan {   // the opaque handle of include/mi355_spmv.h
    mi355::Plan p;
    int acquired_on = -1;  // device of a plan handed out by mi355_spmv_plan_acquire (-1: an ordinary plan)
    int asked_kind = -1;   // the kind the caller named (MI355_KIND_AUTO: p.kind is what was picked)
};

namespace mi355 {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// One retired scratch buffer per device, kept for the next plan: the one-shot entry points (a plan per call,
// the life cycle of the reference's kinds) would otherwise pay a hipMalloc + hipFree — the latter an implicit
// device synchronisation — on every SpMV.  Only a plan whose stream has been synchronised retires its buffer
// here (one_shot); mi355_spmv_plan_destroy keeps hipFree's semantics.
struct RetiredScratch { void* ptr; size_t bytes; };
static std::mutex g_retired_mutex;
static RetiredScratch g_retired[64] = {};

static void* take_retired(size_t bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(g_retired_mutex);
    RetiredScratch& r = g_retired[dev];
    if (!r.ptr || r.bytes < bytes || r.bytes > 4 * bytes + (1u << 20)) return nullptr;
    void* ptr = r.ptr;
    r.ptr = nullptr;
    return ptr;
}

static void retire_scratch(void* ptr, size_t bytes) {
    int dev = 0;
    void* old = nullptr;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) {
        std::lock_guard<std::mutex> lock(g_retired_mutex);
        old = g_retired[dev].ptr;
        g_retired[dev] = RetiredScratch{ptr, bytes};
    } else {
        old = ptr;
    }
    if (old) (void)hipFree(old);
}

static int plan_alloc_scratch(Plan& p) {
    const size_t val_bytes = p.val_type == MI355_VAL_F64 ? 8 : 4;
    size_t off = 0;
    size_t o_tile_nnz = 0, o_tile_row = 0, o_carry_row = 0, o_carry_val = 0, o_counters = 0;
    if (p.kind == MI355_KIND_MERGE) {
        o_tile_nnz = off;  off = align_up(off + sizeof(int64_t) * size_t(p.n_tiles + 1), 256);
        o_tile_row = off;  off = align_up(off + sizeof(int32_t) * size_t(p.n_tiles + 1), 256);
        o_carry_row = off; off = align_up(off + sizeof(int32_t) * size_t(p.n_tiles + 1), 256);
        o_carry_val = off; off = align_up(off + val_bytes * size_t(p.n_tiles + 1), 256);
    } else if (p.kind == MI355_KIND_LIGHT) {
        o_counters = off;  off = align_up(off + 128 * size_t(kXcds + 1), 256);   // 8 shards + the leavers' count
    }
    size_t o_chunk_row = 0;
    if (p.balanced) { o_chunk_row = off; off = align_up(off + sizeof(int32_t) * size_t(p.n_chunks + 1), 256); }
    size_t o_giant_row = 0, o_giant_first = 0, o_giant_partial = 0;
    if (p.n_giant > 0) {
        o_giant_row = off;     off = align_up(off + sizeof(int32_t) * size_t(p.n_giant), 256);
        o_giant_first = off;   off = align_up(off + sizeof(int64_t) * size_t(p.n_giant + 1), 256);
        o_giant_partial = off; off = align_up(off + val_bytes * size_t(p.n_giant_slices), 256);
    }
    p.scratch_bytes = off;
    p.scratch = nullptr;
    if (off) {
        p.scratch_capacity = off;
        p.scratch = take_retired(off);
        if (!p.scratch) MI355_HIP_TRY(hipMalloc(&p.scratch, off));
        char* base = static_cast<char*>(p.scratch);
        p.tile_nnz = reinterpret_cast<int64_t*>(base + o_tile_nnz);
        p.tile_row = reinterpret_cast<int32_t*>(base + o_tile_row);
        p.carry_row = reinterpret_cast<int32_t*>(base + o_carry_row);
        p.carry_val = base + o_carry_val;
        p.counters = reinterpret_cast<unsigned long long*>(base + o_counters);
        if (p.balanced) p.chunk_row = reinterpret_cast<int32_t*>(base + o_chunk_row);
        if (p.n_giant > 0) {
            p.giant_row = reinterpret_cast<int32_t*>(base + o_giant_row);
            p.giant_slice_first = reinterpret_cast<int64_t*>(base + o_giant_first);
            p.giant_partial = base + o_giant_partial;
        }
        if (p.kind == MI355_KIND_LIGHT) {   // zero once; the kernel re-arms the counters at the end of every execute
            MI355_HIP_TRY(hipMemset(p.counters, 0, 128 * size_t(kXcds + 1)));
            MI355_HIP_TRY(hipStreamSynchronize(nullptr));   // the first execute may come on any stream
        }
    }
    return MI355_SPMV_OK;
}

template <typename val_t, typename off_t>
static int execute_typed(Plan& p, const off_t* Ap, const void* Ax, const void* x, void* y, hipStream_t s) {
    const val_t* ax = static_cast<const val_t*>(Ax);
    const val_t* xx = static_cast<const val_t*>(x);
    val_t* yy = static_cast<val_t*>(y);
    switch (p.kind) {
        case MI355_KIND_VECTOR:
            if constexpr (sizeof(val_t) == 4) {   // (a 16-bit matrix under fp32 vectors: plan_create_typed)
                if (p.mat_type == MI355_VAL_F16) return launch_vector_half<off_t, _Float16>(p, Ap, static_cast<const _Float16*>(Ax), xx, yy, s);
                if (p.mat_type == MI355_VAL_BF16) return launch_vector_half<off_t, Bf16>(p, Ap, static_cast<const Bf16*>(Ax), xx, yy, s);
            }
            return launch_rows<VectorRows, off_t, val_t>(p, Ap, ax, xx, yy, s);
        case MI355_KIND_MERGE:
            if (p.mat_type == MI355_VAL_PATTERN) return launch_merge<off_t, val_t, PatternOnes>(p, Ap, nullptr, xx, yy, s);
            if constexpr (sizeof(val_t) == 8)
                if (p.mat_type == MI355_VAL_F32) return launch_merge<off_t, val_t, float>(p, Ap, static_cast<const float*>(Ax), xx, yy, s);
            return launch_merge<off_t, val_t, val_t>(p, Ap, ax, xx, yy, s);
        case MI355_KIND_LIGHT: return launch_rows<LightRows, off_t, val_t>(p, Ap, ax, xx, yy, s);
    }
    set_error("unknown kind %d", p.kind);
    return MI355_SPMV_EINVAL;
}

// The one-shot entry points keep their last few plans (the reference re-creates everything per call, and
// its harness calls a kind 2 000 times in a row on the same matrix, main.cu:102-113 — plan creation, two small kernels and
// two host round trips, is ~90 us of a 270 us call on the target and six times the kernel on the cant stand-in).  A plan is
// found again by the POINTERS and sizes of the structure arrays, the types, the kind and the device.  That is safe when the
// caller has rewritten Ap / Aj in place or re-used the addresses for another matrix of the same sizes: everything a plan
// holds about the structure is a launch-shape decision with a fallback in the kernels (columns outside a window are
// gathered from memory, rows longer than a step finish in the long-row passes, chunk tables are row partitions whatever
// the rows hold, merge coordinates are recomputed by every execute) — except the list of giant rows, so a plan that has
// one is never kept.  MI355_SPMV_PLAN_CACHE=0 turns it off; mi355_spmv_cache_release() frees what it holds.
struct OneShotKey {
    int device, kind, off_type, val_type;
    int32_t n_rows, n_cols;
    int64_t nnz;
    const void *Ap, *Aj;
    bool operator==(const OneShotKey& o) const {
        return device == o.device && kind == o.kind && off_type == o.off_type && val_type == o.val_type && n_rows == o.n_rows &&
               n_cols == o.n_cols && nnz == o.nnz && Ap == o.Ap && Aj == o.Aj;
    }
};
struct OneShotSlot { OneShotKey key; mi355_spmv_plan* plan = nullptr; };
constexpr int kOneShotSlots = 6;
static std::mutex g_oneshot_mutex;
static OneShotSlot g_oneshot[kOneShotSlots];
static int g_oneshot_next = 0;

static bool oneshot_cache_enabled() { return knobs().plan_cache != 0; }

static mi355_spmv_plan* oneshot_take(const OneShotKey& key) {
    std::lock_guard<std::mutex> lock(g_oneshot_mutex);
    for (OneShotSlot& s : g_oneshot)
        if (s.plan && s.key == key) {
            mi355_spmv_plan* p = s.plan;
            s.plan = nullptr;          // (taken OUT: a second thread with the same matrix makes its own plan)
            return p;
        }
    return nullptr;
}

static void oneshot_keep(const OneShotKey& key, mi355_spmv_plan* plan) {
    mi355_spmv_plan* evicted = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_oneshot_mutex);
        OneShotSlot* slot = nullptr;
        for (OneShotSlot& s : g_oneshot)
            if (!s.plan) { slot = &s; break; }
        if (!slot) {
            slot = &g_oneshot[g_oneshot_next];
            g_oneshot_next = (g_oneshot_next + 1) % kOneShotSlots;
            evicted = slot->plan;
        }
        slot->key = key;
        slot->plan = plan;
    }
    if (evicted) (void)mi355_spmv_plan_destroy(evicted);
}

static void oneshot_release_all() {
    mi355_spmv_plan* held[kOneShotSlots];
    {
        std::lock_guard<std::mutex> lock(g_oneshot_mutex);
        for (int i = 0; i < kOneShotSlots; ++i) { held[i] = g_oneshot[i].plan; g_oneshot[i].plan = nullptr; }
    }
    for (mi355_spmv_plan* p : held)
        if (p) (void)mi355_spmv_plan_destroy(p);
}

static OneShotKey key_of(const mi355_spmv_plan* h) {
    const Plan& p = h->p;
    return OneShotKey{h->acquired_on, h->asked_kind >= 0 ? h->asked_kind : p.kind, p.off_type, p.val_type, p.n_rows, p.n_cols, p.nnz, p.Ap, p.Aj};
}

// a kept plan for this matrix, or a new one
static int plan_acquire(mi355_spmv_plan** out, int kind, int off_type, int val_type, int32_t n_rows, int32_t n_cols,
                        int64_t nnz, const void* Ap, const int32_t* Aj) {
    OneShotKey key{-1, kind, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj};
    const bool cache = oneshot_cache_enabled() && nnz > 0 && hipGetDevice(&key.device) == hipSuccess;
    *out = cache ? oneshot_take(key) : nullptr;
    if (*out) return MI355_SPMV_OK;
    // (NO_INDEX_COPY: a kept plan is found again by pointers and must stay right for arrays rewritten in place, so it may
    // hold nothing derived from the contents of Aj)
    const int st = mi355_spmv_plan_create(out, kind, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, MI355_PLAN_NO_INDEX_COPY);
    if (st == MI355_SPMV_OK && cache) (*out)->acquired_on = key.device;
    return st;
}

// give it back: kept for the next call on this matrix when that is safe (see above), destroyed otherwise.  The caller
// has synchronised the stream the plan ran on.  ok = the execute succeeded.
static int plan_release(mi355_spmv_plan* plan, bool ok) {
    if (!plan) return MI355_SPMV_OK;
    if (ok && plan->acquired_on >= 0 && plan->p.n_giant == 0 && plan->p.alpha == 1.0 && plan->p.beta == 0.0) {
        oneshot_keep(key_of(plan), plan);
        return MI355_SPMV_OK;
    }
    if (ok && plan->p.scratch) {          // ... or let at least its scratch serve the next call
        retire_scratch(plan->p.scratch, plan->p.scratch_capacity);
        plan->p.scratch = nullptr;
    }
    return mi355_spmv_plan_destroy(plan);
}

static int one_shot(int kind, int off_type, int val_type, int32_t n_rows, int32_t n_cols, int64_t nnz,
                    const void* Ap, const int32_t* Aj, const void* Ax, const void* x, void* y, void* stream,
                    int semiring = MI355_SEMIRING_PLUS_TIMES) {
    mi355_spmv_plan* plan = nullptr;
    int st = plan_acquire(&plan, kind, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj);
    if (st != MI355_SPMV_OK) return st;
    if (semiring != plan->p.semiring) {
        st = mi355_spmv_plan_set_semiring(plan, semiring);
        if (st != MI355_SPMV_OK) { mi355_spmv_plan_destroy(plan); return st; }
    }
    st = mi355_spmv_plan_execute(plan, Ax, x, y, stream);
    if (st == MI355_SPMV_OK) {
        hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
        if (e != hipSuccess) {
            set_error("hipStreamSynchronize -> %s", hipGetErrorString(e));
            st = MI355_SPMV_EHIP;
        }
    }
    const int st2 = plan_release(plan, st == MI355_SPMV_OK);
    return st != MI355_SPMV_OK ? st : st2;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_spmv_version(void) { return MI355_SPMV_VERSION; }

const char* mi355_spmv_status_string(int status) {
    switch (status) {
        case MI355_SPMV_OK: return "ok";
        case MI355_SPMV_EINVAL: return "invalid argument";
        case MI355_SPMV_ENOTSUP: return "not supported";
        case MI355_SPMV_EHIP: return "HIP runtime error";
        case MI355_SPMV_ENOMEM: return "out of device memory";
        case MI355_SPMV_ENODEV: return "no gfx950 device";
    }
    return "unknown status";
}

const char* mi355_spmv_last_error(void) { return g_err; }

int mi355_spmv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    int found = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++found;
    }
    return found;
}

// Common body of plan_create / plan_create_block.  blk == nullptr: an ordinary plan (Ap[0] == 0).
// blk != nullptr: rows of a larger CSR (Ap[0] = blk->phase in 0..3, nnz = END offset); VECTOR / LIGHT blocks
// inherit the launch shape of the whole matrix's plan (rows_plan.hip, inherit_rows_shape).
static int plan_create_impl(mi355_spmv_plan** out, int kind, int off_type, int val_type, int32_t n_rows,
                            int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj, int flags,
                            const BlockSpec* blk) {
    g_err[0] = 0;
    if (!out) { set_error("plan_create: null plan pointer"); return MI355_SPMV_EINVAL; }
    *out = nullptr;
    if (kind < 0 || kind >= MI355_KIND_COUNT) { set_error("plan_create: unknown kind %d", kind); return MI355_SPMV_EINVAL; }
    if (off_type != MI355_OFF_I32 && off_type != MI355_OFF_I64) { set_error("plan_create: unknown offset type %d", off_type); return MI355_SPMV_EINVAL; }
    if (val_type != MI355_VAL_F32 && val_type != MI355_VAL_F64 && val_type != MI355_VAL_I32) { set_error("plan_create: unknown value type %d", val_type); return MI355_SPMV_EINVAL; }
    if (val_type == MI355_VAL_I32 && kind != MI355_KIND_MERGE) {
        set_error("plan_create: integer values are a feature of the generalized merge kind (as the functor is in the reference)");
        return MI355_SPMV_ENOTSUP;
    }
    if (n_rows < 0 || n_cols < 0 || nnz < 0) { set_error("plan_create: negative size"); return MI355_SPMV_EINVAL; }
    // the kernels step 16-byte groups past a row's end before masking: 32-bit index arithmetic needs headroom
    if (off_type == MI355_OFF_I32 && nnz > INT32_MAX - 4096) { set_error("plan_create: nnz does not fit 32-bit offsets with headroom (use 64-bit offsets)"); return MI355_SPMV_EINVAL; }
    if (n_rows > 0 && !Ap) { set_error("plan_create: null Ap"); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && !Aj) { set_error("plan_create: null Aj"); return MI355_SPMV_EINVAL; }
    if (nnz > 0 && n_cols == 0) { set_error("plan_create: nonzeros but no columns"); return MI355_SPMV_EINVAL; }
    if (blk && (blk->phase < 0 || blk->phase > 3 || blk->phase > nnz)) { set_error("plan_create_block: Ap[0] must be 0..3"); return MI355_SPMV_EINVAL; }

    mi355_spmv_plan* h = new (std::nothrow) mi355_spmv_plan();   // (the plan value-initialised: common.hpp)
    if (!h) { set_error("plan_create: host allocation failed"); return MI355_SPMV_ENOMEM; }
    Plan& p = h->p;
    p.knob = knobs();
    p.kind = kind; p.off_type = off_type; p.val_type = val_type; p.flags = flags;
    p.mat_type = val_type;
    p.n_rows = n_rows; p.n_cols = n_cols; p.nnz = nnz; p.Ap = Ap; p.Aj = Aj;
    p.nnz_begin = blk ? blk->phase : 0;
    p.nnz_read = nnz;
    p.elems_per_lane = 4;
    p.alpha = 1.0;
    p.beta = 0.0;
    ProbeSamples probe;     // plan-time data: dropped when the create returns
    GiantRowList giants;
    int st;
    if (blk && kind != MI355_KIND_MERGE && blk->whole) {
        st = inherit_rows_shape(p, *blk->whole, *blk);
        if (st == MI355_SPMV_OK) st = find_giant_rows(p, giants);
        if (st == MI355_SPMV_OK) set_rows_launch(p);
    } else {
        st = probe_structure(p, probe);          // one tiny kernel + one 16-byte copy (synchronises)
        if (st == MI355_SPMV_OK) {
            if (kind == MI355_KIND_MERGE) shape_merge(p, probe);
            else st = shape_rows(p, probe, giants);   // (synchronises)
        }
    }
    if (st != MI355_SPMV_OK) { delete h; return st; }
    st = plan_alloc_scratch(p);
    if (st == MI355_SPMV_OK) st = build_chunk_table(p, giants);
    if (st == MI355_SPMV_OK) st = build_packed_index(p);
    if (st != MI355_SPMV_OK) {
        if (p.packed_index) (void)hipFree(p.packed_index);
        if (p.scratch) (void)hipFree(p.scratch);
        delete h;
        return st;
    }
    *out = h;
    return MI355_SPMV_OK;
}

int mi355_spmv_plan_create(mi355_spmv_plan** out, int kind, int off_type, int val_type, int32_t n_rows,
                           int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj, int flags) {
    if (kind != MI355_KIND_AUTO) {
        const int st = plan_create_impl(out, kind, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, flags, nullptr);
        if (st == MI355_SPMV_OK) (*out)->asked_kind = kind;
        return st;
    }
    // MI355_KIND_AUTO (include/mi355_spmv.h): integer values exist for MERGE only; otherwise the VECTOR plan's own
    // analysis says whether the rows are skewed (decide_balance: the chunks had to be cut by weight) — then merge-path
    // is the kind to run (web-Google stand-in 45 vs 71 us, R-MAT-24 2.43 vs 2.82 ms), else VECTOR stays.
    int st = plan_create_impl(out, val_type == MI355_VAL_I32 ? MI355_KIND_MERGE : MI355_KIND_VECTOR, off_type, val_type,
                              n_rows, n_cols, nnz, Ap, Aj, flags, nullptr);
    if (st == MI355_SPMV_OK && (*out)->p.kind == MI355_KIND_VECTOR && (*out)->p.balanced) {
        (void)mi355_spmv_plan_destroy(*out);
        st = plan_create_impl(out, MI355_KIND_MERGE, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj, flags, nullptr);
    }
    if (st == MI355_SPMV_OK) (*out)->asked_kind = MI355_KIND_AUTO;
    return st;
}

int mi355_spmv_plan_create_block(mi355_spmv_plan** out, int kind, int off_type, int val_type,
                                 const mi355_spmv_plan_shape* whole, int64_t row_begin, int64_t chunk_begin,
                                 int64_t n_chunks, int64_t nnz_begin_whole, int32_t n_rows, int32_t n_cols,
                                 int64_t nnz_end, const void* Ap, const int32_t* Aj, int flags) {
    BlockSpec blk{whole, row_begin, chunk_begin, n_chunks, nnz_begin_whole, int(nnz_begin_whole & 3)};
    if (n_rows == 0) { blk.phase = 0; nnz_end = 0; }   // an empty block owns no element of its view
    return plan_create_impl(out, kind, off_type, val_type, n_rows, n_cols, nnz_end, Ap, Aj, flags, &blk);
}

int mi355_spmv_plan_create_typed(mi355_spmv_plan** out, int kind, int off_type, int mat_type, int x_type, int y_type,
                                 int32_t n_rows, int32_t n_cols, int64_t nnz, const void* Ap, const int32_t* Aj, int flags) {
    g_err[0] = 0;
    if (out) *out = nullptr;
    const auto known = [](int t) { return t == MI355_VAL_F32 || t == MI355_VAL_F64 || t == MI355_VAL_I32; };
    const bool pattern = mat_type == MI355_VAL_PATTERN;        // (a matrix type only: never the type of x or y)
    const bool half = is_half_matrix(mat_type);                // (F16 / BF16: matrix types only as well)
    if ((!known(mat_type) && !pattern && !half) || !known(x_type) || !known(y_type)) { set_error("plan_create_typed: unknown value type"); return MI355_SPMV_EINVAL; }
    if (x_type != y_type) { set_error("plan_create_typed: x and y of different types are not built"); return MI355_SPMV_ENOTSUP; }
    if (pattern) {
        if (kind == MI355_KIND_AUTO) kind = MI355_KIND_MERGE;
        if (kind != MI355_KIND_MERGE) {
            if (kind < 0 || kind >= MI355_KIND_COUNT) { set_error("plan_create_typed: unknown kind %d", kind); return MI355_SPMV_EINVAL; }
            set_error("plan_create_typed: pattern matrices are built for the merge kind only (as integers, semirings and mixed value types are)");
            return MI355_SPMV_ENOTSUP;
        }
        // shaped exactly as the valued plan of x's type (same tiles, runs and window) ...
        const int st = plan_create_impl(out, kind, off_type, x_type, n_rows, n_cols, nnz, Ap, Aj, flags, nullptr);
        if (st != MI355_SPMV_OK) return st;
        Plan& p = (*out)->p;
        p.mat_type = MI355_VAL_PATTERN;
        (*out)->asked_kind = kind;
        // ... but every execute walks the tiles: the row-parallel run kernel such a shape may name has no pattern form
        merge_report_tile_walk(p);
        return st;
    }
    if (mat_type == x_type) return mi355_spmv_plan_create(out, kind, off_type, x_type, n_rows, n_cols, nnz, Ap, Aj, flags);
    if (half) {
        if (x_type != MI355_VAL_F32) {
            set_error("plan_create_typed: a 16-bit matrix is built under fp32 x and y only");
            return MI355_SPMV_ENOTSUP;
        }
        if (kind == MI355_KIND_AUTO) kind = MI355_KIND_VECTOR;
        if (kind != MI355_KIND_VECTOR) {
            if (kind < 0 || kind >= MI355_KIND_COUNT) { set_error("plan_create_typed: unknown kind %d", kind); return MI355_SPMV_EINVAL; }
            set_error("plan_create_typed: 16-bit matrix values are built for the vector kind only (the kind whose banded plans are bound by the matrix stream)");
            return MI355_SPMV_ENOTSUP;
        }
        // shaped exactly as the fp32 plan of the same structure and flags, packed index included ...
        const int st = plan_create_impl(out, kind, off_type, x_type, n_rows, n_cols, nnz, Ap, Aj, flags, nullptr);
        if (st != MI355_SPMV_OK) return st;
        Plan& p = (*out)->p;
        p.mat_type = mat_type;
        (*out)->asked_kind = kind;
        // ... and reported as what executes: a shape the 16-bit chunked kernels are not built for runs the plain kernel
        set_half_matrix_launch(p);
        return st;
    }
    if (!(mat_type == MI355_VAL_F32 && x_type == MI355_VAL_F64)) {
        set_error("plan_create_typed: the only mixed combination built is an fp32 matrix under fp64 vectors");
        return MI355_SPMV_ENOTSUP;
    }
    if (kind == MI355_KIND_AUTO) kind = MI355_KIND_MERGE;
    if (kind != MI355_KIND_MERGE) {
        set_error("plan_create_typed: mixed value types are built for the merge kind only (the kind the reference generalizes)");
        return MI355_SPMV_ENOTSUP;
    }
    const int st = plan_create_impl(out, kind, off_type, x_type, n_rows, n_cols, nnz, Ap, Aj, flags, nullptr);
    if (st == MI355_SPMV_OK) (*out)->p.mat_type = mat_type;
    return st;
}

int mi355_spmv_plan_get_shape(const mi355_spmv_plan* h, mi355_spmv_plan_shape* sh) {
    if (!h || !sh) { set_error("plan_get_shape: null argument"); return MI355_SPMV_EINVAL; }
    export_rows_shape(h->p, sh);
    return MI355_SPMV_OK;
}

int mi355_spmv_plan_partition(const mi355_spmv_plan* h, int parts, int64_t* row_cuts, int64_t* chunk_cuts,
                              int64_t* nnz_cuts) {
    g_err[0] = 0;
    if (!h || parts < 1 || !row_cuts || !chunk_cuts || !nnz_cuts) { set_error("plan_partition: bad argument"); return MI355_SPMV_EINVAL; }
    return partition_plan(h->p, parts, row_cuts, chunk_cuts, nnz_cuts);
}

int mi355_spmv_knobs_reload(void) {
    knobs_reload();
    oneshot_release_all();     // (the kept one-shot plans were shaped under the old knobs)
    return MI355_SPMV_OK;
}

int mi355_spmv_cache_release(void) {
    oneshot_release_all();
    return MI355_SPMV_OK;
}

int mi355_spmv_plan_acquire(mi355_spmv_plan** out, int kind, int off_type, int val_type, int32_t n_rows, int32_t n_cols,
                            int64_t nnz, const void* Ap, const int32_t* Aj) {
    g_err[0] = 0;
    if (!out) { set_error("plan_acquire: null pointer"); return MI355_SPMV_EINVAL; }
    return plan_acquire(out, kind, off_type, val_type, n_rows, n_cols, nnz, Ap, Aj);
}

int mi355_spmv_plan_release(mi355_spmv_plan* plan, int executed_ok) { return plan_release(plan, executed_ok != 0); }

int mi355_spmv_plan_execute(mi355_spmv_plan* h, const void* Ax, const void* x, void* y, void* stream) {
    g_err[0] = 0;
    if (!h) { set_error("plan_execute: null plan"); return MI355_SPMV_EINVAL; }
    Plan& p = h->p;
    const bool pattern = p.mat_type == MI355_VAL_PATTERN;      // (MERGE only: Ax is ignored and may be NULL)
    if (p.nnz > 0 && ((!Ax && !pattern) || !x)) { set_error("plan_execute: null Ax or x"); return MI355_SPMV_EINVAL; }
    if (p.n_rows > 0 && !y) { set_error("plan_execute: null y"); return MI355_SPMV_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_offsets(p, [&](auto* Ap) -> int {
        using off_t = std::remove_cv_t<std::remove_pointer_t<decltype(Ap)>>;
        if (p.val_type == MI355_VAL_I32) {      // (MERGE only: plan_create refuses the other kinds)
            const int32_t* xx = static_cast<const int32_t*>(x);
            int32_t* yy = static_cast<int32_t*>(y);
            if (pattern) return launch_merge<off_t, int32_t, PatternOnes>(p, Ap, nullptr, xx, yy, s);
            return launch_merge<off_t, int32_t, int32_t>(p, Ap, static_cast<const int32_t*>(Ax), xx, yy, s);
        }
        return p.val_type == MI355_VAL_F32 ? execute_typed<float>(p, Ap, Ax, x, y, s) : execute_typed<double>(p, Ap, Ax, x, y, s);
    });
}

int mi355_spmv_plan_destroy(mi355_spmv_plan* h) {
    if (!h) return MI355_SPMV_OK;
    int st = MI355_SPMV_OK;
    if (h->p.scratch) {
        hipError_t e = hipFree(h->p.scratch);
        if (e != hipSuccess) { set_error("hipFree -> %s", hipGetErrorString(e)); st = MI355_SPMV_EHIP; }
    }
    if (h->p.packed_index) {
        hipError_t e = hipFree(h->p.packed_index);
        if (e != hipSuccess) { set_error("hipFree -> %s", hipGetErrorString(e)); st = MI355_SPMV_EHIP; }
    }
    delete h;
    return st;
}

int mi355_spmv_plan_set_semiring(mi355_spmv_plan* h, int semiring) {
    g_err[0] = 0;
    if (!h) { set_error("plan_set_semiring: null plan"); return MI355_SPMV_EINVAL; }
    if (semiring < 0 || semiring >= MI355_SEMIRING_COUNT) { set_error("plan_set_semiring: unknown semiring %d", semiring); return MI355_SPMV_EINVAL; }
    if (h->p.kind != MI355_KIND_MERGE && semiring != MI355_SEMIRING_PLUS_TIMES) {
        set_error("plan_set_semiring: only the merge kind is generalized (as in the reference)");
        return MI355_SPMV_ENOTSUP;
    }
    if (semiring != MI355_SEMIRING_PLUS_TIMES && (h->p.alpha != 1.0 || h->p.beta != 0.0)) {
        set_error("plan_set_semiring: alpha/beta are set; they are defined for (+, *) only");
        return MI355_SPMV_ENOTSUP;
    }
    h->p.semiring = semiring;
    return MI355_SPMV_OK;
}

int mi355_spmv_plan_set_alpha_beta(mi355_spmv_plan* h, double alpha, double beta) {
    g_err[0] = 0;
    if (!h) { set_error("plan_set_alpha_beta: null plan"); return MI355_SPMV_EINVAL; }
    if (h->p.semiring != MI355_SEMIRING_PLUS_TIMES && (alpha != 1.0 || beta != 0.0)) {
        set_error("plan_set_alpha_beta: scaling is defined for the (+, *) semiring only");
        return MI355_SPMV_ENOTSUP;
    }
    if (h->p.val_type == MI355_VAL_I32 && (alpha != 1.0 || beta != 0.0)) {
        set_error("plan_set_alpha_beta: not for integer values");
        return MI355_SPMV_ENOTSUP;
    }
    h->p.alpha = alpha;
    h->p.beta = beta;
    return MI355_SPMV_OK;
}

int mi355_spmv_stream_synchronize(void* stream) {
    g_err[0] = 0;
    MI355_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return MI355_SPMV_OK;
}

int mi355_spmv_plan_get_info(const mi355_spmv_plan* h, mi355_spmv_plan_info* info) {
    if (!h || !info) { set_error("plan_get_info: null argument"); return MI355_SPMV_EINVAL; }
    const Plan& p = h->p;
    memset(info, 0, sizeof(*info));
    info->kind = p.kind; info->off_type = p.off_type; info->val_type = p.val_type;
    info->lanes_per_row = p.lanes_per_row;
    info->elems_per_lane = p.elems_per_lane;
    info->block_threads = (p.kind == MI355_KIND_MERGE && p.merge_rows && p.mat_type != MI355_VAL_PATTERN)
                              ? p.mr_block : (p.block_threads > 0 ? p.block_threads : kBlock);
    info->grid_blocks = p.grid_blocks;
    info->tile_items = p.tile_items;
    info->n_tiles = p.n_tiles;
    info->rows_per_chunk = p.rows_per_chunk;
    info->scratch_bytes = (int64_t)(p.scratch_bytes + p.packed_bytes);
    info->packed_index_bytes = (int64_t)p.packed_bytes;
    info->packed_index_escapes = p.packed_escapes;
    info->n_kernels = p.n_kernels;
    // (a 16-bit-matrix plan on the plain kernel stages no window, whatever the shape it shares with the fp32 plan holds)
    const bool windowed = p.window_elems > 0 && !(is_half_matrix(p.mat_type) && !half_matrix_chunked(p));
    info->window_elems = windowed ? p.window_elems : 0;
    info->window_segments = windowed ? (p.n_seg >= 2 ? p.n_seg : 1) : 0;
    snprintf(info->main_kernel, sizeof(info->main_kernel), "%s", p.main_kernel);
    info->balanced_chunks = p.balanced ? 1 : 0;
    info->rows_cap = p.rows_cap;
    info->n_chunks = p.n_chunks;
    snprintf(info->knobs, sizeof(info->knobs), "%s", p.knob.text);
    return MI355_SPMV_OK;
}

int mi355_spmv_plan_get_mat_type(const mi355_spmv_plan* h, int* mat_type) {
    if (!h || !mat_type) { set_error("plan_get_mat_type: null argument"); return MI355_SPMV_EINVAL; }
    *mat_type = h->p.mat_type;
    return MI355_SPMV_OK;
}

int mi355_spmv_narrow_values(int dst_type, int64_t n, const float* src, void* dst, void* stream) {
    g_err[0] = 0;
    if (!is_half_matrix(dst_type)) { set_error("narrow_values: the destination type is MI355_VAL_F16 or MI355_VAL_BF16, not %d", dst_type); return MI355_SPMV_EINVAL; }
    if (n < 0) { set_error("narrow_values: negative size"); return MI355_SPMV_EINVAL; }
    if (n > 0 && (!src || !dst)) { set_error("narrow_values: null src or dst"); return MI355_SPMV_EINVAL; }
    if (n == 0) return MI355_SPMV_OK;
    return launch_narrow_values(dst_type, n, src, dst, static_cast<hipStream_t>(stream));
}

int mi355_spmv_plan_merge_coords(mi355_spmv_plan* h, int64_t* tile_row, int64_t* tile_nnz) {
    if (!h || !tile_row || !tile_nnz) { set_error("plan_merge_coords: null argument"); return MI355_SPMV_EINVAL; }
    Plan& p = h->p;
    if (p.kind != MI355_KIND_MERGE) { set_error("plan_merge_coords: not a merge plan"); return MI355_SPMV_EINVAL; }
    MI355_HIP_TRY(hipDeviceSynchronize());
    if (p.merge_rows) {        // (this plan's executes find run boundaries only: compute all tile coordinates now)
        const int st = merge_compute_coords(p);
        if (st != MI355_SPMV_OK) return st;
    } else if (!p.coords_valid) { set_error("plan_merge_coords: no execute yet"); return MI355_SPMV_EINVAL; }
    const size_t n = size_t(p.n_tiles + 1);
    int32_t* rows32 = new (std::nothrow) int32_t[n];
    if (!rows32) return MI355_SPMV_ENOMEM;
    hipError_t e = hipMemcpy(rows32, p.tile_row, n * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(tile_nnz, p.tile_nnz, n * sizeof(int64_t), hipMemcpyDeviceToHost);
    for (size_t i = 0; i < n; ++i) tile_row[i] = rows32[i];
    delete[] rows32;
    if (e != hipSuccess) { set_error("hipMemcpy -> %s", hipGetErrorString(e)); return MI355_SPMV_EHIP; }
    return MI355_SPMV_OK;
}

#define MI355_SPMV_DEFINE(KIND, KINDENUM, SUF, OFF, OFFENUM, VAL, VALENUM)                            \
    int mi355_spmv_##KIND##_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap,             \
                                  const int32_t* Aj, const VAL* Ax, const VAL* x, VAL* y, void* st) { \
        return one_shot(KINDENUM, OFFENUM, VALENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, Ax, x, y, st); \
    }
#define MI355_SPMV_DEFINE_KIND(KIND, KINDENUM)                                                 \
    MI355_SPMV_DEFINE(KIND, KINDENUM, i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)   \
    MI355_SPMV_DEFINE(KIND, KINDENUM, i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)  \
    MI355_SPMV_DEFINE(KIND, KINDENUM, i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)   \
    MI355_SPMV_DEFINE(KIND, KINDENUM, i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)

#define MI355_SPMV_DEFINE_GENL(SUF, OFF, OFFENUM, VAL, VALENUM)                                          \
    int mi355_spmv_merge_genl_##SUF(int semiring, int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap, \
                                    const int32_t* Aj, const VAL* Ax, const VAL* x, VAL* y, void* st) {  \
        if (semiring < 0 || semiring >= MI355_SEMIRING_COUNT) {                                           \
            set_error("merge_genl: unknown semiring %d", semiring);                                       \
            return MI355_SPMV_EINVAL;                                                                     \
        }                                                                                                 \
        return one_shot(MI355_KIND_MERGE, OFFENUM, VALENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, Ax, x, y, st, semiring); \
    }
MI355_SPMV_DEFINE_GENL(i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_GENL(i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_GENL(i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_GENL(i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_GENL(i32_i32, int32_t, MI355_OFF_I32, int32_t, MI355_VAL_I32)
MI355_SPMV_DEFINE_GENL(i64_i32, int64_t, MI355_OFF_I64, int32_t, MI355_VAL_I32)

#define MI355_SPMV_DEFINE_MIXED(SUF, OFF, OFFENUM)                                                            \
    int mi355_spmv_merge_f32mat_f64vec_##SUF(int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap,             \
                                            const int32_t* Aj, const float* Ax, const double* x, double* y, void* st) { \
        mi355_spmv_plan* plan = nullptr;                                                                         \
        int rc = mi355_spmv_plan_create_typed(&plan, MI355_KIND_MERGE, OFFENUM, MI355_VAL_F32, MI355_VAL_F64,    \
                                              MI355_VAL_F64, n_rows, n_cols, (int64_t)nnz, Ap, Aj, MI355_PLAN_DEFAULT); \
        if (rc != MI355_SPMV_OK) return rc;                                                                      \
        rc = mi355_spmv_plan_execute(plan, Ax, x, y, st);                                                        \
        if (rc == MI355_SPMV_OK) rc = mi355_spmv_stream_synchronize(st);                                         \
        const int rc2 = mi355_spmv_plan_destroy(plan);                                                           \
        return rc != MI355_SPMV_OK ? rc : rc2;                                                                   \
    }
MI355_SPMV_DEFINE_MIXED(i32, int32_t, MI355_OFF_I32)
MI355_SPMV_DEFINE_MIXED(i64, int64_t, MI355_OFF_I64)

// pattern matrices: the arguments of merge_genl without Ax.  A plan per call, as the mixed entry points above: the kept
// one-shot plans are keyed by the vector type alone, and a valued call on the same Ap / Aj must never get this plan.
#define MI355_SPMV_DEFINE_PATTERN(SUF, OFF, OFFENUM, VAL, VALENUM)                                               \
    int mi355_spmv_merge_pattern_##SUF(int semiring, int32_t n_rows, int32_t n_cols, OFF nnz, const OFF* Ap,     \
                                       const int32_t* Aj, const VAL* x, VAL* y, void* st) {                      \
        if (semiring < 0 || semiring >= MI355_SEMIRING_COUNT) {                                                  \
            set_error("merge_pattern: unknown semiring %d", semiring);                                           \
            return MI355_SPMV_EINVAL;                                                                            \
        }                                                                                                        \
        mi355_spmv_plan* plan = nullptr;                                                                         \
        int rc = mi355_spmv_plan_create_typed(&plan, MI355_KIND_MERGE, OFFENUM, MI355_VAL_PATTERN, VALENUM,      \
                                              VALENUM, n_rows, n_cols, (int64_t)nnz, Ap, Aj, MI355_PLAN_DEFAULT); \
        if (rc != MI355_SPMV_OK) return rc;                                                                      \
        rc = mi355_spmv_plan_set_semiring(plan, semiring);                                                       \
        if (rc == MI355_SPMV_OK) rc = mi355_spmv_plan_execute(plan, nullptr, x, y, st);                          \
        if (rc == MI355_SPMV_OK) rc = mi355_spmv_stream_synchronize(st);                                         \
        const int rc2 = mi355_spmv_plan_destroy(plan);                                                           \
        return rc != MI355_SPMV_OK ? rc : rc2;                                                                   \
    }
MI355_SPMV_DEFINE_PATTERN(i32_f32, int32_t, MI355_OFF_I32, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_PATTERN(i32_f64, int32_t, MI355_OFF_I32, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_PATTERN(i32_i32, int32_t, MI355_OFF_I32, int32_t, MI355_VAL_I32)
MI355_SPMV_DEFINE_PATTERN(i64_f32, int64_t, MI355_OFF_I64, float, MI355_VAL_F32)
MI355_SPMV_DEFINE_PATTERN(i64_f64, int64_t, MI355_OFF_I64, double, MI355_VAL_F64)
MI355_SPMV_DEFINE_PATTERN(i64_i32, int64_t, MI355_OFF_I64, int32_t, MI355_VAL_I32)

MI355_SPMV_DEFINE_KIND(vector, MI355_KIND_VECTOR)
MI355_SPMV_DEFINE_KIND(merge, MI355_KIND_MERGE)
MI355_SPMV_DEFINE_KIND(light, MI355_KIND_LIGHT)
MI355_SPMV_DEFINE_KIND(auto, MI355_KIND_AUTO)

}  // extern "C"
