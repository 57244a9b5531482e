/*
 * pt_user_object_n.h -- the CSG node of a user-defined Object subclass whose
 * span iterator yields several spans per ray (pt_object_device_spans;
 * reference include/object.h:14-20: Object::makeSpanIterator returns any
 * SpanIterator, include/span.h:129-171: which yields any number of spans).
 *
 * Appended to a scene's module by codegen.cpp only when the scene holds such
 * an object, after device/pt_device.h, whose node protocol it implements (see
 * Sph there, and UObj in pt_user_object.h for the one-span form): a leaf that
 * owns K consecutive primitive slots, PRIM .. PRIM + K - 1, one per span.  The
 * caller's bodies arrive as B (codegen's UObjB_<id>):
 *     int B::spans(V3 o, V3 d, const float *prm, float *t0, float *t1)
 *         -- the number n of spans, 0 <= n <= K, the ray o + t d (d not
 *            normalised) has with the object; t0[k] <= t1[k] for k < n, in ray
 *            order and strictly separated, t1[k] < t0[k + 1];
 *     V3 B::normal(V3 p, int k, const float *prm)
 *         -- the outward surface normal at the boundary point p of span k
 *            (traceRay flips the end normal, path-trace.h:89).
 * Span j lives in slot PRIM + j; the count is clamped to 0..K and every slot is
 * walked by compile-time index (value selects on the cursor, as PT_PULL_SELECT
 * does for the binary nodes), so a wrong body -- a count too large, unordered
 * spans -- can give wrong pixels and never an access out of range, and no
 * register array is indexed by a runtime value.
 *
 * Fast first-hit (pt_device.h "Every primitive contributes at most one
 * span"): a slot holds at most one span, and the K spans of one ray are
 * strictly separated, so they are what K positive primitives under Unions would
 * contribute when every pair of them passes sep(): the merges hand each of them
 * through unchanged.  The pair checks at the merge nodes above (fast_ok,
 * pair_ok over each_pos), the union rule (cheap_ok: no tie, since separated
 * spans have different starts) and isect_empty (the node's output lies inside
 * the union of its slots' spans) therefore see K ordinary primitives; nothing
 * is checked between the slots of one object, whose separation the body
 * promises.  The other checks are the conservative ones of UObj: never dark,
 * "ends before EPS" only from the computed spans themselves, no Compact / Occl
 * form.  Each slot costs three words of PrimSpans registers per lane.
 */
namespace ptd
{

template <int PRIM, int K, int OFF, int MAT, class B>
struct UObjN
{
    static_assert(K >= 1 && K <= 8, "UObjN: 1..PT_OBJECT_MAX_SPANS slots");
    static constexpr int LO = PRIM, HI = PRIM + K;
    static constexpr bool UNION_ONLY = true; /* a leaf: no Intersection / Difference at or below */
    static constexpr bool NO_DIFF = true;
    template <class PS>
    __device__ static __forceinline__ int isect_empty(const PS &) { return 1; }
    struct Ctx
    {
        V3 o; /* the query origin (in the object's frame) */
    };
    struct St
    {
        float t0[K], t1[K]; /* compile-time indices only */
        int n;              /* live slots: 0 .. n - 1 */
        int cur;            /* the next slot pull() yields */
    };
    __device__ static __forceinline__ void prep(Ctx &c, V3 o, const Env &) { c.o = univ(o); }
    __device__ static __forceinline__ void prep_l(Ctx &c, V3 o, const Env &) { c.o = o; }
    __device__ static __forceinline__ void init(St &s, const Ctx &c, const Ray &q, const Env &e)
    {
        float t0[K], t1[K];
#pragma unroll
        for (int j = 0; j < K; j++)
            t0[j] = t1[j] = __builtin_nanf("");
        const int n = B::spans(c.o, q.d, e.P + OFF, t0, t1);
        s.n = n < 0 ? 0 : n > K ? K : n;
        s.cur = 0;
#pragma unroll
        for (int j = 0; j < K; j++)
            s.t0[j] = t0[j], s.t1[j] = t1[j];
    }
    __device__ static __forceinline__ bool pull(St &s, CS &out)
    {
        const int k = s.cur;
        if (k >= s.n)
            return false;
        float a = s.t0[0], b = s.t1[0];
#pragma unroll
        for (int j = 1; j < K; j++) {
            const bool here = k == j;
            a = here ? s.t0[j] : a, b = here ? s.t1[j] : b;
        }
        out.t0 = a, out.t1 = b;
        out.r0 = mkref(PRIM + k, MAT, 0), out.r1 = mkref(PRIM + k, MAT, 1);
        s.cur = k + 1;
        return true;
    }
    template <class PS>
    __device__ static __forceinline__ void span(PS &ps, const Ctx &c, const Ray &q, const Env &e)
    {
        St s;
        init(s, c, q, e);
#pragma unroll
        for (int j = 0; j < K; j++)
            ps.t0[PRIM + j] = s.t0[j], ps.t1[PRIM + j] = s.t1[j], ps.live[PRIM + j] = j < s.n ? 1 : 0;
    }
    /* init() from the slots span() filled: the live ones are the first n */
    template <class PS>
    __device__ static __forceinline__ void init_ps(St &s, const PS &ps)
    {
        int n = 0;
#pragma unroll
        for (int j = 0; j < K; j++)
            s.t0[j] = ps.t0[PRIM + j], s.t1[j] = ps.t1[PRIM + j], n += ps.live[PRIM + j];
        s.n = n;
        s.cur = 0;
    }
    template <int J, class F>
    __device__ static __forceinline__ void each_slot(F &f)
    {
        if constexpr (J < K) {
            f(IC<PRIM + J>(), IC<MAT>());
            each_slot<J + 1>(f);
        }
    }
    template <class F>
    __device__ static __forceinline__ void each_pos(F &&f) { each_slot<0>(f); }
    template <class SEL, class PS>
    __device__ static __forceinline__ void span_sel(PS &ps, const Ctx &c, const Ray &q, const Env &e)
    {
        if constexpr (SEL::take(MAT))
            span(ps, c, q, e);
    }
    template <class SEL, class F>
    __device__ static __forceinline__ void each_sel(F &&f)
    {
        if constexpr (SEL::take(MAT))
            each_slot<0>(f);
    }
    /* lanes whose every slot is dead or ends before EPS, from the spans themselves */
    template <class SEL, bool NORM>
    __device__ static __forceinline__ u64 clear_mask(const Ctx &c, const Ray &q, const Env &e)
    {
        if constexpr (SEL::take(MAT))
            return ~0ull;
        St s;
        init(s, c, q, e);
        int clear = 1;
#pragma unroll
        for (int j = 0; j < K; j++)
            clear &= (j >= s.n) | (s.t1[j] < EPS);
        return __ballot(clear != 0);
    }
    template <class SEL>
    __device__ static constexpr bool clear_ok() { return true; }
    template <class PS, bool D = false>
    __device__ static __forceinline__ int fast_ok(const PS &) { return 1; }
    __device__ static __forceinline__ V3 normal(int prim, float t, V3 o, V3 d, const Env &e)
    {
        return B::normal(o + t * d, prim - PRIM, e.P + OFF);
    }
    template <class SEL>
    __device__ static constexpr bool raw_ok() { return true; }
    template <class SEL>
    __device__ static constexpr int nsel() { return SEL::take(MAT) ? K : 0; }
    /* no direction is provably dark for an emissive shape the kernel cannot see into */
    template <class SEL>
    __device__ static __forceinline__ u64 dark_mask(const Ctx &, V3, const Env &)
    {
        if constexpr (!SEL::take(MAT))
            return ~0ull;
        return 0ull;
    }
    template <class SEL>
    __device__ static __forceinline__ bool dark_pre(const Ctx &, const Env &)
    {
        return true;
    }
};

} // namespace ptd
