// functor_texts.inc — TEST CODE: the functors of tests/functor_cases.py, written the way a user of the reference writes
// a functor_t (merge_genl.cuh:19-38).  ONE definition for both executions: tests/functor_cases.py reads this file as TEXT
// and hands it to sp.Functor (hiprtc, the device), tests/cpp/functor_sim.cpp includes it for the host simulation.
// y of 1 byte (OrAndFn<.., unsigned char>), 2 (MinI16Fn), 4, 6 (Tri), 8, 12 (Stat12) and 16 bytes (Stat16).
template <typename M, typename X, typename Y>
struct PlusTimesFn {
    __host__ __device__ __forceinline__ static Y initialize() { return Y(0); }
    __host__ __device__ __forceinline__ static Y combine(const M& a, const X& x) { return Y(a * x); }
    __host__ __device__ __forceinline__ static Y reduce(const Y& l, const Y& r) { return l + r; }
};
template <typename M, typename X, typename Y>
struct MinPlusFn {
    __device__ static Y initialize() { return Y(INFINITY); }
    __device__ static Y combine(const M& a, const X& x) { return Y(a + x); }
    __device__ static Y reduce(const Y& l, const Y& r) { return r < l ? r : l; }
};
template <typename M, typename X, typename Y>
struct MaxTimesFn {
    __device__ static Y initialize() { return Y(-INFINITY); }
    __device__ static Y combine(const M& a, const X& x) { return Y(a * x); }
    __device__ static Y reduce(const Y& l, const Y& r) { return l < r ? r : l; }
};
template <typename M, typename X, typename Y>
struct MaxPlusFn {
    __device__ static Y initialize() { return Y(-INFINITY); }
    __device__ static Y combine(const M& a, const X& x) { return Y(a + x); }
    __device__ static Y reduce(const Y& l, const Y& r) { return l < r ? r : l; }
};
template <typename M, typename X, typename Y>
struct OrAndFn {
    __device__ static Y initialize() { return Y(0); }
    __device__ static Y combine(const M& a, const X& x) { return (a != M(0) && x != X(0)) ? Y(1) : Y(0); }
    __device__ static Y reduce(const Y& l, const Y& r) { return (l != Y(0) || r != Y(0)) ? Y(1) : Y(0); }
};
// (min, +) on 16-bit integers: a y of 2 bytes
struct MinI16Fn {
    __device__ static short initialize() { return 32767; }
    __device__ static short combine(const short& a, const short& x) { return short(a + x); }
    __device__ static short reduce(const short& l, const short& r) { return r < l ? r : l; }
};
// sum, minimum and maximum of a * x in three shorts: a y of 6 bytes (the last shuffled word is half padding)
struct Tri { short sum, lo, hi; };
struct TriFn {
    __device__ static Tri initialize() { Tri t; t.sum = 0; t.lo = 32767; t.hi = -32768; return t; }
    __device__ static Tri combine(const short& a, const short& x) { Tri t; t.sum = t.lo = t.hi = short(a * x); return t; }
    __device__ static Tri reduce(const Tri& l, const Tri& r) {
        Tri t; t.sum = short(l.sum + r.sum); t.lo = r.lo < l.lo ? r.lo : l.lo; t.hi = l.hi < r.hi ? r.hi : l.hi; return t;
    }
};
// maximum, minimum and count: a y of 12 bytes
struct Stat12 { float hi, lo; int count; };
struct Stat12Fn {
    __device__ static Stat12 initialize() { Stat12 s; s.hi = -INFINITY; s.lo = INFINITY; s.count = 0; return s; }
    __device__ static Stat12 combine(const float& a, const float& x) { Stat12 s; s.hi = s.lo = a * x; s.count = 1; return s; }
    __device__ static Stat12 reduce(const Stat12& l, const Stat12& r) {
        Stat12 s; s.hi = l.hi < r.hi ? r.hi : l.hi; s.lo = r.lo < l.lo ? r.lo : l.lo; s.count = l.count + r.count; return s;
    }
};
// sum in fp64, maximum in fp32 and count: a y of 16 bytes, 8-byte aligned
struct Stat16 { double sum; float hi; int count; };
struct Stat16Fn {
    __device__ static Stat16 initialize() { Stat16 s; s.sum = 0; s.hi = -INFINITY; s.count = 0; return s; }
    __device__ static Stat16 combine(const float& a, const double& x) { Stat16 s; s.sum = a * x; s.hi = float(a * x); s.count = 1; return s; }
    __device__ static Stat16 reduce(const Stat16& l, const Stat16& r) {
        Stat16 s; s.sum = l.sum + r.sum; s.hi = l.hi < r.hi ? r.hi : l.hi; s.count = l.count + r.count; return s;
    }
};
// five independent types (spmv.h:29-34): int32 indices, int64 offsets, an fp64 matrix, an int32 x, an int64 y: the sum
// of the products (every element counts) plus a million per product above 2.5 (the count of tests/test_gpu_functor.py)
struct CountAbove {
    __device__ static long long initialize() { return 0; }
    __device__ static long long combine(const double& a, const int& x) { return (long long)(a * x) + (a * x > 2.5 ? 1000000 : 0); }
    __device__ static long long reduce(const long long& l, const long long& r) { return l + r; }
};
