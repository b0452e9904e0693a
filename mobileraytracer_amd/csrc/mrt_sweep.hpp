// mrt_sweep.hpp - sweep queries (mrt_sweep_spheres_device): the sweep functions, shared by the host
// (mrt_sphere_sweep) and the kernels, and the per-lane walk that minimises them.
//
// The motion.  A sphere of radius r has its centre at c(t) = o + d * t, each component one multiply and one
// add (sweepCentre).  d is taken as given, not normalised: with d = goal - start, t is the fraction of the
// motion.  The answer for a ray is DEFINED as the least, in the total order (t, kind, input index), of the
// functions below over the candidates whose t is below the ray's bound and not NaN.  Every translation unit
// compiles with -ffp-contract=off, so host and device give the same bits.
//
// Valid input: o, d, r finite and r >= 0; anything else accepts nothing.  d == 0 is valid (so is a d whose
// squared length underflows to 0: it counts as no motion): only the start test can accept.  r == 0 is a
// moving point; its answer is THIS function's - a t validated by distance, a contact within the slack
// below of the surface - and not the Moller-Trumbore bits of mrt_cast_rays_device.
//
// sweepTriangle(A, AB, AC, o, d, r), for triangles and area lights.  Every dot is mrt::dot ((x + y) + z).
//   0. Start test: dist(o).d2 <= r * r gives t = 0 (and d2 below +inf: an overflow accepts nothing).  dist is
//      sweepPointTriangle below: pointTriangle's record unless an edge's or the face's own is nearer.
//   1. dd = d . d; dd == 0: a miss.  ap = o - A, so that sizes matter and the scene's offset does not.
//   2. Up to seven candidate times, the times at which the centre reaches distance r from a feature's
//      CARRIER, each max(root, 0) wherever the motion reaches the carrier at some parameter >= 0 (a root
//      that rounding pushed just below 0 must not lose a contact at the start):
//      the face's plane  n = cross(AB, AC); nn = n . n (nn == 0: none); s0 = n . ap; nd = n . d;
//                        approaching only (s0 > 0 and nd < 0, or s0 < 0 and nd > 0):
//                        root = (|s0| - r * sqrtf(nn)) / |nd|
//      a corner P        (P - A = 0, AB, AC)   m = (P - A) - ap; tca = (m . d) / dd; w = m - d * tca;
//                        disc = r * r - w . w (disc < 0: none); h = sqrtf(disc / dd);
//                        tca + h >= 0: root = tca - h
//      an edge P, e      (0, AB; 0, AC; AB, AC - AB)   ee = e . e (ee == 0: none); m as above;
//                        mp = m - e * ((m . e) / ee); dp = d - e * ((d . e) / ee); ddp = dp . dp (0: none:
//                        the motion is parallel to the line); tca = (mp . dp) / ddp; w = mp - dp * tca;
//                        disc, h and root as for a corner with ddp for dd
//      This is the closest-approach form: w is the perpendicular offset of the carrier from the centre's
//      path as a vector, and the discriminant is r^2 - |w|^2.  The textbook b^2 - a c loses about
//      eps L^2 / r near grazing (L the distance travelled), which for a small sphere far from its start is
//      far more than eps M; here the error of w is eps L and that of the discriminant eps L r.
//   3. Validation.  The carriers do not decide which feature is touched; the distance function does.  The
//      candidates are taken in ascending order (equal times once); candidate tk is valid when, with
//      ck = c(tk), dist(ck).d2 <= acc2 (and below +inf), where
//          acc = r * (1 + 2^-20) + (kSweepK * eps) * M,   acc2 = acc * acc,   eps = 2^-24,
//      M the largest |coordinate| of o, ck and the corners A, fl(A + AB), fl(A + AC).  The first valid
//      candidate is the answer; the record is dist's own at ck (contact point q, barycentrics
//      u, v) plus the centre ck.  No feature-membership test with its own rounding exists, so a contact
//      is never attributed to a feature the distance function would not confirm.  The function is total
//      on finite input.  `limit`: candidates strictly above it are not validated (the host passes +inf;
//      a lane passes the time it has to beat, which cannot change the lane's answer).
// sweepPlane(normal, point, o, d, r): s0 = normal . (o - point); start test s0 * s0 <= r * r; else with
//   nd = normal . d, approaching only, t = max((|s0| - r) / |nd|, 0), validated by pointPlane(ck).d2 <= acc2
//   with M over o, ck and point.
// sweepSphere(C, sqRadius, o, d, r), the sphere's SURFACE as pointSphere and boxSphere mean it:
//   start test pointSphere(o).d2 <= r * r; else m = C - o, len2 = m . m, R = sqrtf(sqRadius), tca and w as
//   for a corner; from outside (len2 >= sqRadius) the first root against R + r: disc = (R + r)^2 - w . w
//   (< 0: none), tca + h >= 0: t = max(tca - h, 0); from inside the exit root against R - r:
//   disc = max((R - r)^2 - w . w, 0), t = max(tca + h, 0); validated by pointSphere(ck).d2 <= acc2 with M
//   over o, ck, C and R.
//
// The slack kSweepK.  A candidate's centre misses distance r by the error of its time times the speed
// towards the surface, which the closest-approach form keeps to a few eps (L + M), and by the distance
// function's own error.  Measured on tests/test_sweep_cpu.py's pairs: planes and spheres, which have one
// carrier, are validated at |sqrt(d2) - r| <= 6.4 eps M; for triangles a slack of 8 eps M still confirms
// every first contact of the sphere shrunk by 8 eps M.  kSweepK = 32 is that 8 with a margin of 4.
//
// The contract, on valid finite input against a float64 evaluation on the stored float32 values, M the
// largest |coordinate| of the start, of the centre at the time compared, of the corners, and r:
//   (a) never late:  the returned t (for a miss, +inf or the bound) is at most the exact first-contact time
//       of the sphere shrunk to radius r - g eps M;
//   (b) never early: at a returned hit the exact distance from the reported centre to the primitive is at
//       most r + g eps M.
// Two-sided so that it holds at grazing contacts, where t itself is ill-conditioned.  g = kSweepG below is
// MEASURED (the smallest power of two for which both sides hold on every pair of the test, which pins 4 g);
// (a) needs 16 for triangles and 8 for planes and spheres, (b) 38.2 for triangles - the slack itself plus
// 2^-20 r - and 6.5 for planes and spheres.  The late pairs at smaller g spread over the decades of L / r
// (0.1 .. 100) as the pairs themselves do: g does not depend on L / r there.  The kernel uses nothing from g.
//
// The walk (sweepRay): planes, spheres and area lights one by one, then the triangles - under BVH a descent
// of the reference tree (triNodes / triRootRef), near child first by entry parameter, the far child pushed
// with its entry parameter and compared again when popped; under Naive a loop in input order.
//
// The cull is certified.  An accepted candidate has dist(ck).d2 <= acc2, q a point of the triangle.  By the nearest-point
// lemma (mrt_nearest.hpp) ck is then, on every axis, within sqrt(acc2) + 2 c1 of every reference box above
// the triangle, c1 = kNearestK eps M'.  With Mr the largest |coordinate| of o, the root box and r, every
// such ck has |coordinate| <= Mr + r (1 + 2^-20) + (kSweepK + 2 kNearestK) eps X, X = max(|ck|, Mr), hence
// X <= 2.1 Mr <= Mc = 4 Mr, and M, M' <= Mc.  So the per-axis distance is at most
//     (r (1 + 2^-20) + (kSweepK + 2 kNearestK) eps Mc) (1 + 3 eps)          (three roundings of acc2)
// and sweepCullR = (r + (kSweepK + 2 kNearestK + 4) eps Mc) (1 + 2^-19) is above that after its own three
// roundings; the 4 eps Mc are for the slab test: two for rounding mn - R and mx + R, one for the rounding of
// ck's own sum, one for the rounding of the difference to o.  fl(o + fl(d * s)) is monotone in s per axis.
// So per axis with d.a > 0 (d.a < 0 mirrored), lo = mn.a - R, hi = mx.a + R:
//     in  = ((lo - o.a) / d.a) * (1 - 2^-20)   is at most every s >= 0 with c(s).a >= mn.a - R (true R),
//     out = ((hi - o.a) / d.a) * (1 + 2^-20)   is at least every s >= 0 with c(s).a <= mx.a + R,
// (the 2^-20 cover the product's, the quotient's and the factor's roundings, barring underflow), and a
// zero d.a is a plain interval compare of o.a against lo and hi.  A node is skipped only when the largest
// in (and 0) is strictly above the smallest out, or strictly above the lane's limit min(bound, best t):
// then no s in [0, limit] has the centre inside the box grown by R.  Every compare is strict and false for
// NaN (a NaN in or out constrains nothing; a non-finite Mr never culls), so a box entered exactly at the
// best t is still visited and an earlier-ordered tie still wins.  As for the nearest-point cull, a scene
// with a NaN first corner is outside the BVH = Naive guarantee (the builder replaces a NaN bound by the
// next box's: mrt_overlap.hpp).
#pragma once

#include "mrt_nearest.hpp"

namespace mrt {

constexpr float kSweepK = 32.0F;  // the validation slack in eps M (four times the measured candidate error)
constexpr float kSweepG = 64.0F;  // the contract's g as measured (tests/test_sweep_cpu.py pins 4 g)
constexpr int kSweepThreads = kNearestThreads;  // one wave per workgroup: 4 KB of stack in LDS

struct SweepHit {
    bool hit;
    float t;       // the first-contact time; +inf on a miss
    v3 c;          // the centre at t
    PointDist pd;  // the distance function's record at c: contact point q, barycentrics u, v
};

MRT_HD bool sweepFinite(float x) { return fabsf(x) < __builtin_inff(); }  // false for NaN
MRT_HD bool sweepValid(v3 o, v3 d, float r) {
    return sweepFinite(o.x) && sweepFinite(o.y) && sweepFinite(o.z) && sweepFinite(d.x) && sweepFinite(d.y) &&
           sweepFinite(d.z) && sweepFinite(r) && r >= 0.0F;
}
MRT_HD v3 sweepCentre(v3 o, v3 d, float t) { return o + d * t; }
MRT_HD float sweepAbsMax(float m, v3 a) { return fmaxf(fmaxf(m, fabsf(a.x)), fmaxf(fabsf(a.y), fabsf(a.z))); }
// d2 <= lim and d2 < +inf: false for NaN, and an overflow accepts nothing
MRT_HD bool sweepWithin(float d2, float lim) { return d2 <= lim && d2 < __builtin_inff(); }
MRT_HD float sweepAcc2(float r, float M) {
    const float acc = r * (1.0F + 9.5367431640625e-07F) + (kSweepK * 5.9604644775390625e-08F) * M;
    return acc * acc;
}
MRT_HD SweepHit sweepMiss() {
    return SweepHit{false, __builtin_inff(), v3{0.0F, 0.0F, 0.0F}, PointDist{0.0F, v3{0.0F, 0.0F, 0.0F}, 0.0F, 0.0F}};
}
constexpr float kSweepNone = __builtin_nanf("");  // an absent candidate: no compare holds for it

// the time at which a point moving as -m + d * s reaches distance sqrt(r2) from the origin of m's frame
// (m: from the start to the carrier, perpendicular part only for a line), first root; dd = d . d > 0
MRT_HD float sweepRoot(v3 m, v3 d, float dd, float r2) {
    const float tca = dot(m, d) / dd;
    const v3 w = m - d * tca;
    const float disc = r2 - dot(w, w);
    if (!(disc >= 0.0F)) return kSweepNone;
    const float h = sqrtf(disc / dd);
    if (!(tca + h >= 0.0F)) return kSweepNone;
    return fmaxf(tca - h, 0.0F);
}
MRT_HD float sweepEdgeRoot(v3 m, v3 e, v3 d, float r2) {
    const float ee = dot(e, e);
    if (!(ee > 0.0F)) return kSweepNone;
    const v3 mp = m - e * (dot(m, e) / ee);
    const v3 dp = d - e * (dot(d, e) / ee);
    const float ddp = dot(dp, dp);
    if (!(ddp > 0.0F)) return kSweepNone;
    return sweepRoot(mp, dp, ddp, r2);
}

// The sweep's distance function for a triangle: pointTriangle's record, or the nearest of four more records
// where one of them is strictly nearer - the three edges' and the face's by its normal.  pointTriangle's
// region tests and face weights are differences of products of size^4 whose true value is the squared area
// (va, vb, vc), so its point is off along the triangle by about eps size / sin^2 (sin the sine of the angle at
// A): for a thin triangle that is a distance error of (that)^2 / (2 r) at a contact, hundreds of eps M at
// sin = 0.01, and for a sliver the point may be far from the closest one.  A point-segment distance has no
// such cancellation, and the weights by the normal (below) lose eps / sin only.  Every record is a point of
// the triangle in pointTriangle's own form q = (A + AB * u) + AC * v with 0 <= u, v and u + v <= 1, its d2
// computed from that q, so the nearest-point lemma covers it and (b) holds by construction.
//   AB: s = clamp(d1 / (AB . AB)): (s, 0);  AC: s = clamp(d2 / (AC . AC)): (0, s);
//   BC: e = AC - AB, s = clamp((e . bp) / (e . e)): (1 - s, s);   clamp(x) = fminf(fmaxf(x, 0), 1), NaN -> 0
//   face: n = cross(AB, AC); u = (cross(ap, AC) . n) / (n . n); v = (cross(AB, ap) . n) / (n . n); taken
//   when u >= 0, v >= 0 and u + v <= 1 (false for NaN: a segment or a point has no face)
MRT_HD PointDist sweepEdgePoint(v3 A, v3 AB, v3 AC, v3 p, float u, float v, PointDist best) {
    PointDist r;
    r.q = (A + AB * u) + AC * v;
    const v3 e = p - r.q;
    r.d2 = (e.x * e.x + e.y * e.y) + e.z * e.z;
    r.u = u;
    r.v = v;
    return r.d2 < best.d2 ? r : best;
}
MRT_HD float sweepClamp01(float x) { return fminf(fmaxf(x, 0.0F), 1.0F); }
MRT_HD PointDist sweepPointTriangle(v3 A, v3 AB, v3 AC, v3 p) {
    PointDist r = pointTriangle(A, AB, AC, p);
    const v3 ap = p - A;
    r = sweepEdgePoint(A, AB, AC, p, sweepClamp01(dot(AB, ap) / dot(AB, AB)), 0.0F, r);
    r = sweepEdgePoint(A, AB, AC, p, 0.0F, sweepClamp01(dot(AC, ap) / dot(AC, AC)), r);
    const v3 bc = AC - AB;
    const float s = sweepClamp01(dot(bc, ap - AB) / dot(bc, bc));
    r = sweepEdgePoint(A, AB, AC, p, 1.0F - s, s, r);
    const v3 n = cross(AB, AC);
    const float nn = dot(n, n);
    const float u = dot(cross(ap, AC), n) / nn, v = dot(cross(AB, ap), n) / nn;
    if (u >= 0.0F && v >= 0.0F && u + v <= 1.0F) r = sweepEdgePoint(A, AB, AC, p, u, v, r);
    return r;
}

MRT_HD SweepHit sweepTriangle(v3 A, v3 AB, v3 AC, v3 o, v3 d, float r, float limit) {
    SweepHit h = sweepMiss();
    if (!sweepValid(o, d, r)) return h;
    const float r2 = r * r;
    const PointDist p0 = sweepPointTriangle(A, AB, AC, o);
    if (sweepWithin(p0.d2, r2)) {
        h.hit = true;
        h.t = 0.0F;
        h.c = sweepCentre(o, d, 0.0F);
        h.pd = sweepPointTriangle(A, AB, AC, h.c);
        return h;
    }
    const float dd = dot(d, d);
    if (!(dd > 0.0F)) return h;
    const v3 ap = o - A;
    float tk[7];
    {
        const v3 n = cross(AB, AC);
        const float nn = dot(n, n), s0 = dot(n, ap), nd = dot(n, d);
        tk[0] = kSweepNone;
        if (nn > 0.0F && ((s0 > 0.0F && nd < 0.0F) || (s0 < 0.0F && nd > 0.0F)))
            tk[0] = fmaxf((fabsf(s0) - r * sqrtf(nn)) / fabsf(nd), 0.0F);
    }
    const v3 mA = v3{0.0F, 0.0F, 0.0F} - ap, mB = AB - ap, mC = AC - ap;
    tk[1] = sweepEdgeRoot(mA, AB, d, r2);
    tk[2] = sweepEdgeRoot(mA, AC, d, r2);
    tk[3] = sweepEdgeRoot(mB, AC - AB, d, r2);
    tk[4] = sweepRoot(mA, d, dd, r2);
    tk[5] = sweepRoot(mB, d, dd, r2);
    tk[6] = sweepRoot(mC, d, dd, r2);
    float mTri = sweepAbsMax(0.0F, A);
    mTri = sweepAbsMax(mTri, A + AB);
    mTri = sweepAbsMax(mTri, A + AC);
    mTri = sweepAbsMax(mTri, o);
    float last = -1.0F;  // (every candidate is >= 0)
    for (int it = 0; it < 7; ++it) {
        float t = __builtin_inff();
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (tk[k] > last && tk[k] < t) t = tk[k];
        if (!(t < __builtin_inff()) || t > limit) return h;
        const v3 c = sweepCentre(o, d, t);
        const PointDist pd = sweepPointTriangle(A, AB, AC, c);
        if (sweepWithin(pd.d2, sweepAcc2(r, sweepAbsMax(mTri, c)))) {
            h.hit = true;
            h.t = t;
            h.c = c;
            h.pd = pd;
            return h;
        }
        last = t;
    }
    return h;
}

MRT_HD SweepHit sweepPlane(v3 normal, v3 point, v3 o, v3 d, float r, float limit) {
    SweepHit h = sweepMiss();
    if (!sweepValid(o, d, r)) return h;
    const float s0 = dot(normal, o - point);
    float t = 0.0F, lim = r * r;
    if (!sweepWithin(s0 * s0, lim)) {
        const float nd = dot(normal, d);
        if (!((s0 > 0.0F && nd < 0.0F) || (s0 < 0.0F && nd > 0.0F))) return h;
        t = fmaxf((fabsf(s0) - r) / fabsf(nd), 0.0F);
        if (!(t < __builtin_inff()) || t > limit) return h;
        lim = -1.0F;  // (validated below, against acc2)
    }
    const v3 c = sweepCentre(o, d, t);
    const PointDist pd = pointPlane(normal, point, c);
    if (lim < 0.0F) lim = sweepAcc2(r, sweepAbsMax(sweepAbsMax(sweepAbsMax(0.0F, o), point), c));
    if (!sweepWithin(pd.d2, lim)) return h;
    h.hit = true;
    h.t = t;
    h.c = c;
    h.pd = pd;
    return h;
}

MRT_HD SweepHit sweepSphere(v3 C, float sqRadius, v3 o, v3 d, float r, float limit) {
    SweepHit h = sweepMiss();
    if (!sweepValid(o, d, r)) return h;
    const float r2 = r * r;
    const PointDist p0 = pointSphere(C, sqRadius, o);
    if (sweepWithin(p0.d2, r2)) {
        h.hit = true;
        h.t = 0.0F;
        h.c = sweepCentre(o, d, 0.0F);
        h.pd = pointSphere(C, sqRadius, h.c);
        return h;
    }
    const float dd = dot(d, d);
    if (!(dd > 0.0F)) return h;
    const v3 m = C - o;
    const float R = sqrtf(sqRadius);
    float t;
    if (dot(m, m) >= sqRadius) {
        const float Rr = R + r;
        t = sweepRoot(m, d, dd, Rr * Rr);
    } else {
        const float Rr = R - r;
        const float tca = dot(m, d) / dd;
        const v3 w = m - d * tca;
        const float disc = fmaxf(Rr * Rr - dot(w, w), 0.0F);
        t = fmaxf(tca + sqrtf(disc / dd), 0.0F);
    }
    if (!(t < __builtin_inff()) || t > limit) return h;  // (a NaN t: no candidate)
    const v3 c = sweepCentre(o, d, t);
    const PointDist pd = pointSphere(C, sqRadius, c);
    const float M = fmaxf(sweepAbsMax(sweepAbsMax(sweepAbsMax(0.0F, o), C), c), R);
    if (!sweepWithin(pd.d2, sweepAcc2(r, M))) return h;
    h.hit = true;
    h.t = t;
    h.c = c;
    h.pd = pd;
    return h;
}

// mrt_sphere_sweep / mrt_kat_sphere_sweep: pair i of a kind (mrt_point_distance's kinds and layouts) against
// the sweep o xyz, d xyz, r
MRT_HD SweepHit sweepPrim(int kind, const float* f, const float* ray) {
    const v3 o{ray[0], ray[1], ray[2]}, d{ray[3], ray[4], ray[5]};
    const float r = ray[6], lim = __builtin_inff();
    if (kind == 1) return sweepPlane(v3{f[0], f[1], f[2]}, v3{f[3], f[4], f[5]}, o, d, r, lim);
    if (kind == 2) return sweepSphere(v3{f[0], f[1], f[2]}, f[3], o, d, r, lim);
    return sweepTriangle(v3{f[0], f[1], f[2]}, v3{f[3], f[4], f[5]}, v3{f[6], f[7], f[8]}, o, d, r, lim);
}

// the cull's radius (see above): Mr the largest |coordinate| of o, the box above the triangles, and r
MRT_HD float sweepCullR(float r, float Mr) {
    const float Mc = 4.0F * Mr;
    return (r + ((kSweepK + 2.0F * kNearestK + 4.0F) * 5.9604644775390625e-08F) * Mc) * (1.0F + 1.9073486328125e-06F);
}

// The held answer of one lane: the best candidate so far (code: BVH-order, kNoPrim none) and the time a
// candidate must beat (t; the ray's bound while nothing is held).
struct SweepBest {
    float t;
    uint32_t code;
    v3 c, q;
    float u, v;
    int tests;
};

// A candidate replaces the held one when it is earlier, or bit-equal and earlier in (kind, input index); a
// miss is never accepted, nor a time at or above the bound while nothing is held.
__device__ __forceinline__ void sweepOffer(const QueryTables& tb, const SweepHit& c, uint32_t code, SweepBest& sb) {
    ++sb.tests;
    if (!c.hit) return;
    bool take = c.t < sb.t;
    if (!take && c.t == sb.t && sb.code != kNoPrim) {
        const uint32_t kc = primKind(code), kh = primKind(sb.code);
        take = kc != kh ? kc < kh : nearestInput(tb, code) < nearestInput(tb, sb.code);
    }
    if (!take) return;
    sb.t = c.t;
    sb.code = code;
    sb.c = c.c;
    sb.q = c.pd.q;
    sb.u = c.pd.u;
    sb.v = c.pd.v;
}

__device__ __forceinline__ void sweepTri(const DScene& s, const QueryTables& tb, int j, v3 o, v3 d, float r, uint32_t src,
                                         SweepBest& sb) {
    const uint32_t code = encodePrim(kTriangle, static_cast<uint32_t>(j));
    if (code == src) return;
    const float4* g = s.triGeom + 3 * j;
    sweepOffer(tb, sweepTriangle(xyz(ld4(g)), xyz(ld4(g + 1)), xyz(ld4(g + 2)), o, d, r, sb.t), code, sb);
}

// The conservative slab test of the cull (see above): false when no s in [0, limit] has the centre inside
// the box grown by R; *entry: the parameter the far child is pushed with.
__device__ __forceinline__ bool sweepSlab(float mnx, float mny, float mnz, float mxx, float mxy, float mxz, v3 o, v3 d,
                                          float R, float limit, float* entry) {
    const float mn[3] = {mnx, mny, mnz}, mx[3] = {mxx, mxy, mxz};
    const float oo[3] = {o.x, o.y, o.z}, dv[3] = {d.x, d.y, d.z};
    float in = 0.0F, out = limit;
    bool apart = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = mn[a] - R, hi = mx[a] + R;
        if (dv[a] == 0.0F) {
            apart = apart || oo[a] < lo || oo[a] > hi;
            continue;
        }
        const bool pos = dv[a] > 0.0F;
        const float ad = fabsf(dv[a]);
        const float xin = pos ? lo - oo[a] : oo[a] - hi;
        const float xout = pos ? hi - oo[a] : oo[a] - lo;
        const float ein = (xin / ad) * (1.0F - 9.5367431640625e-07F);
        const float eout = (xout / ad) * (1.0F + 9.5367431640625e-07F);
        if (ein > in) in = ein;
        if (eout < out) out = eout;
    }
    *entry = in;
    return !(apart || in > out);
}

// The reference tree, near child first.  Stack: TStack (reference and entry parameter per entry).
template <bool kHit, class Stack>
__device__ __forceinline__ void sweepTriangles(const DScene& s, const QueryTables& tb, v3 o, v3 d, float r, uint32_t src,
                                               SweepBest& sb, Stack& st) {
    const GRoot& root = s.triRootRef;
    if (root.count == 0) return;
    float m = fabsf(o.x);
    m = absMaxNan(m, o.y);
    m = absMaxNan(m, o.z);
    m = absMaxNan(m, r);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        m = absMaxNan(m, root.bmin[a]);
        m = absMaxNan(m, root.bmax[a]);
    }
    const float R = sweepCullR(r, m);
    float e;
    if (!sweepSlab(root.bmin[0], root.bmin[1], root.bmin[2], root.bmax[0], root.bmax[1], root.bmax[2], o, d, R, sb.t, &e))
        return;
    const int base = st.sp;
    int ref = root.ref;
    while (true) {
        if (ref >= 0) {
            const float4* np = reinterpret_cast<const float4*>(s.triNodes + ref);
            const float4 n0 = np[0], n1 = np[1], n2 = np[2];
            const int4 n3 = reinterpret_cast<const int4*>(np)[3];
            float el, er;
            const bool goL = sweepSlab(n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, o, d, R, sb.t, &el);
            const bool goR = sweepSlab(n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, o, d, R, sb.t, &er);
            if (goL && goR) {
                const bool leftNear = el <= er;
                st.push(leftNear ? n3.y : n3.x, leftNear ? er : el);
                ref = leftNear ? n3.x : n3.y;
                continue;
            }
            if (goL) {
                ref = n3.x;
                continue;
            }
            if (goR) {
                ref = n3.y;
                continue;
            }
        } else {
            const int first = leafFirst(ref), count = leafCount(ref);
            for (int k = 0; k < count; ++k) {
                sweepTri(s, tb, first + k, o, d, r, src, sb);
                if (kHit && sb.code != kNoPrim) {
                    st.sp = base;  // (what is left on the stack is dropped)
                    return;
                }
            }
        }
        bool found = false;
        while (st.sp != base) {  // the far children, against the limit as it is now
            const int2 en = st.pop();
            if (__int_as_float(en.y) > sb.t) continue;
            ref = en.x;
            found = true;
            break;
        }
        if (!found) return;
    }
}

// The answer of one ray.  bound: the largest t wanted (+inf unbounded, 0 finds nothing).  kHit: only `hit`
// is wanted, so the walk stops at the ray's first acceptance.  One block per kind, each reading through its
// own base pointer (mrt_neighbours.hpp records why).
template <bool kHit, class Stack>
__device__ __forceinline__ SweepBest sweepRay(const DScene& s, const QueryTables& tb, v3 o, v3 d, float r, float bound,
                                              uint32_t src, Stack& st) {
    SweepBest sb{bound, kNoPrim, v3{0.0F, 0.0F, 0.0F}, v3{0.0F, 0.0F, 0.0F}, 0.0F, 0.0F, 0};
    if (!sweepValid(o, d, r)) return sb;  // (accepts nothing and costs no evaluation)
    const bool accel = s.accel == kAccBVH || s.accel == kAccNaive;  // else the lights only
    if (accel) {
        for (int j = 0; j < s.planeRoot.count; ++j) {
            const uint32_t code = encodePrim(kPlane, static_cast<uint32_t>(j));
            if (code == src) continue;
            sweepOffer(tb, sweepPlane(xyz(s.planes[2 * j]), xyz(s.planes[2 * j + 1]), o, d, r, sb.t), code, sb);
            if (kHit && sb.code != kNoPrim) return sb;
        }
        for (int j = 0; j < s.sphereRoot.count; ++j) {
            const float4 c4 = s.spheres[2 * j];
            sweepOffer(tb, sweepSphere(xyz(c4), c4.w, o, d, r, sb.t), encodePrim(kSphere, static_cast<uint32_t>(j)), sb);
            if (kHit && sb.code != kNoPrim) return sb;
        }
    }
    for (int j = 0; j < s.nLights; ++j) {
        const float4* l = s.lights + 4 * j;
        const float4 a4 = l[0];
        if (__float_as_int(a4.w) != 1) continue;  // point lights are never candidates
        sweepOffer(tb, sweepTriangle(xyz(a4), xyz(l[1]), xyz(l[2]), o, d, r, sb.t), encodePrim(kLight, static_cast<uint32_t>(j)),
                   sb);
        if (kHit && sb.code != kNoPrim) return sb;
    }
    if (s.accel == kAccBVH) {
        sweepTriangles<kHit>(s, tb, o, d, r, src, sb, st);
    } else if (s.accel == kAccNaive) {
        for (int i = 0; i < s.triRoot.count; ++i) {
            sweepTri(s, tb, s.triNaive[i], o, d, r, src, sb);
            if (kHit && sb.code != kNoPrim) return sb;
        }
    }
    return sb;
}
}  // namespace mrt
