// mrt_triangle_overlap.hpp - triangle overlap queries (mrt_overlap_triangles_device): the overlap functions of
// a query TRIANGLE, shared by the host (mrt_triangle_overlap) and the kernels, and the per-lane walk that lists
// what they accept.  The narrow phase next to mrt_overlap.hpp's broad phase: which surfaces a mesh's own
// triangles touch, and - with degenerate input - which surfaces a segment touches or a point lies on.
//
// The answer for a query triangle is DEFINED by the functions below: a candidate is accepted when its kind's
// function returns true.  Every translation unit compiles with -ffp-contract=off, so host and device give the
// same bits.  A query triangle is three corners Q0, Q1, Q2, taken as given; a scene triangle is the stored
// A, AB, AC with corners P0 = A, P1 = fl(A + AB), P2 = fl(A + AC), as boxTriangle forms them.  If any of the
// corners is not finite the functions return false.  Degenerate triangles are valid on both sides: the query
// may be a segment or a point, the scene triangle may have zero area.
//
// triTriangle(A, AB, AC, Q0, Q1, Q2), a 23-axis separating-axis test in centred form, boxTriangle's steps.
// Every dot product is mrt::dot ((x + y) + z), every cross product mrt::cross.
//   0. validity (above).
//   1. the hulls, no slack: loP / hiP = the per-axis min / max of P0, P1, P2, loQ / hiQ of Q0, Q1, Q2;
//      boxesApart(loP, hiP, loQ, hiQ) - strict, false for NaN: false.  The only step the cull relies on.
//   2. c = lo * 0.5 + hi * 0.5 with lo = min(loP, loQ), hi = max(hiP, hiQ): the centre of the hull of both.
//      p_k = P_k - c, q_k = Q_k - c.  M = the largest |coordinate| of the six corners; W = the largest
//      |component| of the six centred corners.
//   3. the edges, on the STORED corners (one rounding each, and the query's do not depend on the candidate):
//      e0 = P1 - P0, e1 = P2 - P1, e2 = P0 - P2; f0 = Q1 - Q0, f1 = Q2 - Q1, f2 = Q0 - Q2;
//      nP = cross(e0, e1), nQ = cross(f0, f1).  The 23 axes, IN THE ORDER USED:
//        nP, nQ;   e_i x f_j, i the outer loop, j the inner;   nP x e_i;   nQ x f_j;   nP x f_j;   nQ x e_i.
//      The last twelve are the in-plane edge normals: they make the test complete for coplanar pairs and for
//      a query segment or point in the scene triangle's plane, where the nine e_i x f_j vanish.
//      For an axis a: x_k = a . p_k, y_k = a . q_k, s = (16 eps |a|_1) (M + W), |a|_1 = (|a.x| + |a.y|) + |a.z|;
//        min x > max y + s, or min y > max x + s: false
//      - unless z = ((x0 + x1) + x2) + ((y0 + y1) + y2) is not finite: min / max drop a NaN, so an axis whose
//      projections overflowed (inf - inf) must not reject; with z finite all six are, and the compares are
//      plain.  Every rejecting compare is strict and false for NaN (an overflowed |a|_1 makes s inf or NaN).
//   4. true.
// The result is the AND of independent axis tests: their order is not part of the definition.
// eps = 2^-24, the unit roundoff.
//
// The slack (no false negative).  A separating-axis test is sound for ANY axis (mrt_overlap.hpp): the
// computed edges, normals and products are taken as the axes exactly as they come out, and only the
// projections on them need a bound (barring underflow: every nonzero product is taken to be normal).
// Both triangles are translated by the SAME computed c, and a translation moves no shape relative to the other,
// so c's own rounding is no error at all: with p*_k = P_k - c exactly, |p_k - p*_k| <= eps W per component
// (one rounding of a value of size at most W).  |fl(a . p_k) - a . p*_k| <= |a|_1 (eps W + 3 eps W) to first
// order: the corner's error, and three roundings in the dot product of terms of size at most |a|_inf W.
// Where the exact shapes intersect, min x* <= max y*; so min x <= max y + 8 eps |a|_1 W.  s takes 16: twice
// the first-order need, for the higher-order terms and the roundings of s and of max y + s; and it takes
// (M + W) for W, boxTriangle's form, which keeps the acceptance band proportional to the coordinates' own
// resolution eps M - the corners are known no better - at the price of the false positives measured below.
//
// The false positives the slack admits are MEASURED, not derived: the contract is two-sided, on valid input
// barring underflow -
//   (a) if the two closed shapes intersect in exact arithmetic on the stored float32 corners (touching at a
//       point or along an edge counts), the function returns true: every pair, both shapes degenerate included;
//   (b) if the function returns true, the two shapes are within g eps M of each other - claimed wherever at
//       least one of the two shapes has nonzero area.  For a pair of two degenerate shapes (segment or point
//       against segment or point) every axis but the hulls' may vanish, and only (a) is claimed.
// g = kTriOverlapG below, the smallest power of two that explains every acceptance of
// tests/test_triangle_overlap_cpu.py's pairs (per family and offset in that file's docstring); the test pins
// 4 g.  The kernel uses nothing from g.
//
// triPlane(normal, point, Q0, Q1, Q2): validity (normal, point, corners finite); d_k = Q_k - point;
//   s_k = normal . d_k; slack = (8 eps |normal|_1) (M + D), M over the corners and the point, D the largest
//   |d_k| component; true unless every s_k > slack or every s_k < -slack.  (First-order need
//   eps |normal|_1 (D + 3 D): boxPlane's argument without the half extent.)
// triSphere(centre, sqRadius, Q0, Q1, Q2), the sphere's SURFACE as boxSphere means it: validity (sqRadius finite
//   and >= 0 too); AB = Q1 - Q0, AC = Q2 - Q0; dmin2 = sweepPointTriangle(Q0, AB, AC, centre).d2
//   (mrt_sweep.hpp: the minimum over pointTriangle's record, the three edges' and the face's - bare
//   pointTriangle may overestimate on slivers and would lose a real touch); dmax2 = the largest of
//   |Q_k - centre|^2 ((x x + y y) + z z); R = sqrtf(sqRadius);
//   true unless dmin2 > sweepAcc2(R, M) or dmax2 < sqRadius (1 - kappa), kappa = 8 eps, M over the corners,
//   the centre and R.  sweepAcc2 is the sweep's own validation bound (R (1 + 2^-20) + 32 eps M)^2: the triangle
//   the distance function sees has corners Q0, fl(Q0 + AB), fl(Q0 + AC) with AB and AC rounded once each, off
//   Q1 and Q2 by at most 2 eps M per component each time, under 7 eps M as a distance; the distance function's
//   own error is within 8 eps M (mrt_sweep.hpp, measured); 32 eps M is more than twice the sum.  The far
//   side is boxSphere's: one rounding per difference, square and sum, 8 eps covers the six.
// An area light goes through triTriangle on its A, AB, AC.
//
// The walk (triOverlapQuery): planes, spheres and area lights one by one, then the triangles - under BVH a
// depth-first descent of the reference tree (triNodes / triRootRef; both children overlapping: the right one
// pushed, the left one entered), under Naive the input-order loop.  What depends on the query alone (its
// hull, edges, normal and in-plane normals: TriQuery) is computed once per query.
//
// The cull is the hull compare and nothing finer: a node is skipped only when boxesApart(node box, hull(Q))
// holds - step 1 on a box that contains the scene triangle's hull, exact by the argument of mrt_overlap.hpp
// (and with its exclusion: a scene that holds a triangle whose first corner has a NaN coordinate).  The
// definition is the function's ACCEPTANCE, not exact overlap: a finer cull (boxTriangle(node, Q), say) could
// drop a false positive that (b) admits and Naive reports, and BVH and Naive would disagree.
//
// Cost.  A long diagonal query triangle has a large hull and meets every leaf under it; that is allowed.
// With only `any` wanted the walk stops at a lane's first acceptance; otherwise every accepted candidate is met.
#pragma once

#include "mrt_overlap.hpp"
#include "mrt_sweep.hpp"

namespace mrt {

constexpr float kTriOverlapEps16 = 9.5367431640625e-07F;  // 16 eps = 2^-20: the axis slack's factor
constexpr float kTriOverlapG = 64.0F;  // the measured false-positive distance, in eps M (see above)

// What a query triangle contributes to every pair (step 3's query side), computed once.
struct TriQuery {
    v3 q0, q1, q2;
    v3 lo, hi;        // the hull
    v3 f0, f1, f2;    // the edges
    v3 n;             // nQ
    v3 nf0, nf1, nf2;  // nQ x f_j
    float m;          // the largest |coordinate|
    bool valid;
};

MRT_HD TriQuery triQuery(v3 Q0, v3 Q1, v3 Q2) {
    TriQuery t;
    t.q0 = Q0;
    t.q1 = Q1;
    t.q2 = Q2;
    t.valid = finite3(Q0) && finite3(Q1) && finite3(Q2);
    t.lo = vmin(Q0, vmin(Q1, Q2));
    t.hi = vmax(Q0, vmax(Q1, Q2));
    t.f0 = Q1 - Q0;
    t.f1 = Q2 - Q1;
    t.f2 = Q0 - Q2;
    t.n = cross(t.f0, t.f1);
    t.nf0 = cross(t.n, t.f0);
    t.nf1 = cross(t.n, t.f1);
    t.nf2 = cross(t.n, t.f2);
    t.m = stdmax(normInf(t.lo), normInf(t.hi));
    return t;
}

// step 3 for one axis: p the scene triangle's centred corners, q the query's, mw = M + W
MRT_HD bool triAxisApart(v3 a, v3 p0, v3 p1, v3 p2, v3 q0, v3 q1, v3 q2, float mw) {
    const float x0 = dot(a, p0), x1 = dot(a, p1), x2 = dot(a, p2);
    const float y0 = dot(a, q0), y1 = dot(a, q1), y2 = dot(a, q2);
    const float z = ((x0 + x1) + x2) + ((y0 + y1) + y2);
    const float s = (kTriOverlapEps16 * norm1(a)) * mw;
    const float xmin = stdmin(stdmin(x0, x1), x2), xmax = stdmax(stdmax(x0, x1), x2);
    const float ymin = stdmin(stdmin(y0, y1), y2), ymax = stdmax(stdmax(y0, y1), y2);
    return finiteF(z) && (xmin > ymax + s || ymin > xmax + s);
}

MRT_HD bool triTriangleQ(v3 A, v3 AB, v3 AC, const TriQuery& t) {
    const v3 P0 = A, P1 = A + AB, P2 = A + AC;
    if (!finite3(P0) || !finite3(P1) || !finite3(P2) || !t.valid) return false;
    const v3 loP = vmin(P0, vmin(P1, P2)), hiP = vmax(P0, vmax(P1, P2));
    if (boxesApart(loP.x, loP.y, loP.z, hiP.x, hiP.y, hiP.z, t.lo, t.hi)) return false;
    const v3 c = vmin(loP, t.lo) * 0.5F + vmax(hiP, t.hi) * 0.5F;
    const v3 p0 = P0 - c, p1 = P1 - c, p2 = P2 - c;
    const v3 q0 = t.q0 - c, q1 = t.q1 - c, q2 = t.q2 - c;
    const float M = stdmax(stdmax(normInf(loP), normInf(hiP)), t.m);
    const float W = stdmax(stdmax(stdmax(normInf(p0), normInf(p1)), normInf(p2)),
                           stdmax(stdmax(normInf(q0), normInf(q1)), normInf(q2)));
    const float mw = M + W;
    const v3 e0 = P1 - P0, e1 = P2 - P1, e2 = P0 - P2;
    const v3 nP = cross(e0, e1);
#define MRT_TRI_AXIS(a) \
    if (triAxisApart(a, p0, p1, p2, q0, q1, q2, mw)) return false
    MRT_TRI_AXIS(nP);
    MRT_TRI_AXIS(t.n);
    MRT_TRI_AXIS(cross(e0, t.f0));
    MRT_TRI_AXIS(cross(e0, t.f1));
    MRT_TRI_AXIS(cross(e0, t.f2));
    MRT_TRI_AXIS(cross(e1, t.f0));
    MRT_TRI_AXIS(cross(e1, t.f1));
    MRT_TRI_AXIS(cross(e1, t.f2));
    MRT_TRI_AXIS(cross(e2, t.f0));
    MRT_TRI_AXIS(cross(e2, t.f1));
    MRT_TRI_AXIS(cross(e2, t.f2));
    MRT_TRI_AXIS(cross(nP, e0));
    MRT_TRI_AXIS(cross(nP, e1));
    MRT_TRI_AXIS(cross(nP, e2));
    MRT_TRI_AXIS(t.nf0);
    MRT_TRI_AXIS(t.nf1);
    MRT_TRI_AXIS(t.nf2);
    MRT_TRI_AXIS(cross(nP, t.f0));
    MRT_TRI_AXIS(cross(nP, t.f1));
    MRT_TRI_AXIS(cross(nP, t.f2));
    MRT_TRI_AXIS(cross(t.n, e0));
    MRT_TRI_AXIS(cross(t.n, e1));
    MRT_TRI_AXIS(cross(t.n, e2));
#undef MRT_TRI_AXIS
    return true;
}

MRT_HD bool triTriangle(v3 A, v3 AB, v3 AC, v3 Q0, v3 Q1, v3 Q2) { return triTriangleQ(A, AB, AC, triQuery(Q0, Q1, Q2)); }

MRT_HD bool triPlaneQ(v3 normal, v3 point, const TriQuery& t) {
    if (!finite3(normal) || !finite3(point) || !t.valid) return false;
    const v3 d0 = t.q0 - point, d1 = t.q1 - point, d2 = t.q2 - point;
    const float s0 = dot(normal, d0), s1 = dot(normal, d1), s2 = dot(normal, d2);
    const float M = stdmax(t.m, normInf(point));
    const float D = stdmax(stdmax(normInf(d0), normInf(d1)), normInf(d2));
    const float slack = (kOverlapEps8 * norm1(normal)) * (M + D);
    return !((s0 > slack && s1 > slack && s2 > slack) || (s0 < -slack && s1 < -slack && s2 < -slack));
}

MRT_HD bool triPlane(v3 normal, v3 point, v3 Q0, v3 Q1, v3 Q2) { return triPlaneQ(normal, point, triQuery(Q0, Q1, Q2)); }

MRT_HD bool triSphereQ(v3 centre, float sqRadius, const TriQuery& t) {
    if (!finite3(centre) || !finiteF(sqRadius) || sqRadius < 0.0F || !t.valid) return false;
    const float dmin2 = sweepPointTriangle(t.q0, t.q1 - t.q0, t.q2 - t.q0, centre).d2;
    const v3 g0 = t.q0 - centre, g1 = t.q1 - centre, g2 = t.q2 - centre;
    const float dmax2 = stdmax(stdmax(dot(g0, g0), dot(g1, g1)), dot(g2, g2));
    const float R = sqrtf(sqRadius);
    const float M = stdmax(stdmax(t.m, normInf(centre)), R);
    return !(dmin2 > sweepAcc2(R, M) || dmax2 < sqRadius * (1.0F - kOverlapEps8));
}

MRT_HD bool triSphere(v3 centre, float sqRadius, v3 Q0, v3 Q1, v3 Q2) {
    return triSphereQ(centre, sqRadius, triQuery(Q0, Q1, Q2));
}

// mrt_triangle_overlap / mrt_kat_triangle_overlap: pair i of a kind (mrt_point_distance's kinds and layouts)
// against the triangle (a xyz, b xyz, c xyz) at q
MRT_HD bool triOverlapPrim(int kind, const float* f, const float* q) {
    const v3 Q0{q[0], q[1], q[2]}, Q1{q[3], q[4], q[5]}, Q2{q[6], q[7], q[8]};
    if (kind == 1) return triPlane(v3{f[0], f[1], f[2]}, v3{f[3], f[4], f[5]}, Q0, Q1, Q2);
    if (kind == 2) return triSphere(v3{f[0], f[1], f[2]}, f[3], Q0, Q1, Q2);
    return triTriangle(v3{f[0], f[1], f[2]}, v3{f[3], f[4], f[5]}, v3{f[6], f[7], f[8]}, Q0, Q1, Q2);
}

// One triangle (BVH-order index j); its input index costs one triOrder load, and only when it is accepted.
template <bool kAny>
__device__ __forceinline__ void triOverlapTriangle(const DScene& s, const QueryTables& tb, int j, const TriQuery& t,
                                                   OverlapHeld<kAny>& ol) {
    const float4* g = s.triGeom + 3 * j;
    ++ol.tests;
    if (triTriangleQ(xyz(ld4(g)), xyz(ld4(g + 1)), xyz(ld4(g + 2)), t))
        ol.accept(kAny ? 0u : encodePrim(kTriangle, static_cast<uint32_t>(tb.triOrder[j])));
}

// The reference tree, depth first: overlapTriangles' loop with the query's hull for the box.
template <bool kAny, class Stack>
__device__ __forceinline__ void triOverlapTriangles(const DScene& s, const QueryTables& tb, const TriQuery& t,
                                                    OverlapHeld<kAny>& ol, Stack& st) {
    const GRoot& root = s.triRootRef;
    if (root.count == 0) return;
    if (boxesApart(root.bmin[0], root.bmin[1], root.bmin[2], root.bmax[0], root.bmax[1], root.bmax[2], t.lo, t.hi)) return;
    const int base = st.sp;
    int ref = root.ref;
    while (true) {
        if (ref >= 0) {
            const float4* np = reinterpret_cast<const float4*>(s.triNodes + ref);
            const float4 n0 = np[0], n1 = np[1], n2 = np[2];
            const int4 n3 = reinterpret_cast<const int4*>(np)[3];
            const bool goL = !boxesApart(n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, t.lo, t.hi);
            const bool goR = !boxesApart(n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, t.lo, t.hi);
            if (goL && goR) {
                st.push(n3.y, 0.0F);
                ref = n3.x;
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
                triOverlapTriangle(s, tb, first + k, t, ol);
                if (kAny && ol.count != 0) {
                    st.sp = base;  // (what is left on the stack is dropped)
                    return;
                }
            }
        }
        if (st.sp == base) return;
        ref = st.pop().x;
    }
}

// The accepted set of one query triangle into ol (reset by the caller), overlapBox's order of candidates.  An
// invalid query accepts nothing and costs no evaluation.
template <bool kAny, class Stack>
__device__ __forceinline__ void triOverlapQuery(const DScene& s, const QueryTables& tb, const TriQuery& t,
                                                OverlapHeld<kAny>& ol, Stack& st) {
    if (!t.valid) return;
    const bool accel = s.accel == kAccBVH || s.accel == kAccNaive;  // else the lights only
    if (accel) {
        for (int j = 0; j < s.planeRoot.count; ++j) {
            ++ol.tests;
            if (triPlaneQ(xyz(s.planes[2 * j]), xyz(s.planes[2 * j + 1]), t)) {
                ol.accept(kAny ? 0u : encodePrim(kPlane, static_cast<uint32_t>(tb.planeOrder[j])));
                if (kAny) return;
            }
        }
        for (int j = 0; j < s.sphereRoot.count; ++j) {
            const float4 c4 = s.spheres[2 * j];
            ++ol.tests;
            if (triSphereQ(xyz(c4), c4.w, t)) {
                ol.accept(kAny ? 0u : encodePrim(kSphere, static_cast<uint32_t>(tb.sphereOrder[j])));
                if (kAny) return;
            }
        }
    }
    for (int j = 0; j < s.nLights; ++j) {
        const float4* l = s.lights + 4 * j;
        const float4 a4 = l[0];
        if (__float_as_int(a4.w) != 1) continue;  // point lights are never candidates
        ++ol.tests;
        if (triTriangleQ(xyz(a4), xyz(l[1]), xyz(l[2]), t)) {
            ol.accept(encodePrim(kLight, static_cast<uint32_t>(j)));
            if (kAny) return;
        }
    }
    if (s.accel == kAccBVH) {
        triOverlapTriangles(s, tb, t, ol, st);
    } else if (s.accel == kAccNaive) {
        for (int i = 0; i < s.triRoot.count; ++i) {
            triOverlapTriangle(s, tb, s.triNaive[i], t, ol);
            if (kAny && ol.count != 0) return;
        }
    }
}
}  // namespace mrt
