// mrt_overlap.hpp - overlap queries (mrt_overlap_boxes_device): the overlap functions, shared by the host
// (mrt_box_overlap) and the kernels, and the per-lane walk that lists what they accept.
//
// The answer for a box is DEFINED by the functions below: a candidate is accepted when its kind's
// function returns true.  Every translation unit compiles with -ffp-contract=off, so host and device give
// the same bits.  The reference's Triangle::intersect(const AABB&) (boxIntersect in mrt_grid.cpp) is not
// the definition: it treats each edge as a half-line, and its `inside` term holds for any triangle whose
// plane is parallel to the box diagonal, wherever the triangle lies.
//
// boxTriangle(A, AB, AC, mn, mx), the 13-axis separating-axis test in centred form.  Every dot product is
// mrt::dot ((x + y) + z); every rejecting compare is strict and false for NaN, so an overflow keeps a pair.
//   0. P0 = A, P1 = A + AB, P2 = A + AC (aabbOf's corners).  A corner component or a bound that is not
//      finite, or mn.a > mx.a on some axis: false.  mn == mx is a valid box.
//   1. the hull, no slack: per axis lo = min(P0a, P1a, P2a), hi = max(...); lo > mx.a or hi < mn.a: false.
//   2. c = mn * 0.5 + mx * 0.5; h = mx * 0.5 - mn * 0.5; v_k = P_k - c; e0 = v1 - v0; e1 = v2 - v1;
//      e2 = v0 - v2.  M = the largest |coordinate| of the corners and the bounds; W = the largest |v|
//      component + the largest h component.
//   3. nine axes a = unit_i x e_j, i the outer loop, j the inner (unit_x x e = (0, -e.z, e.y), unit_y x e =
//      (e.z, 0, -e.x), unit_z x e = (-e.y, e.x, 0): exact).  p_k = a . v_k; r = h . |a|;
//      t = r + s, s = (8 eps |a|_1) (M + W), |a|_1 = (|a.x| + |a.y|) + |a.z|;
//      every p_k > t, or every p_k < -t: false.
//   4. n = cross(e0, e1); d = n . v0; q1 = n . v1; q2 = n . v2; spread = max(|q1 - d|, |q2 - d|); r = h . |n|;
//      t = r + s_n, s_n = spread + (16 eps |n|_1) (M + W);
//      d > t or d < -t: false.
//   5. true.
// eps = 2^-24, the unit roundoff.
//
// The slacks (no false negative).  Stars mark exact values on the stored floats.  A separating-axis test is
// sound for ANY axis: if the projections of the triangle and of the box on some vector are disjoint, the two
// are.  So the computed a and n are taken as the axes, exactly as they are, and only the projections on
// them need bounds (barring underflow: every nonzero product is taken to be a normal number):
//   |c - c*| <= eps M and |h - h*| <= eps Wh per component (mn * 0.5 and mx * 0.5 are exact, one rounding);
//   |v - v*| <= eps M + eps Wv (the centre's error, one rounding), Wv + Wh = W;
//   |fl(a . v) - a . v*| <= |a|_1 (eps (M + Wv) + 3 eps Wv) and |fl(h . |a|) - h* . |a|| <= 4 eps |a|_1 Wh
//   to first order, together eps |a|_1 (M + 5 W) <= 4 eps |a|_1 (M + W), since |v| <= 2 M and h <= M give
//   W <= 3 M.  s is twice that: the factor covers the higher-order terms and the roundings of s and r + s.
// For step 4 the triangle's projection on the computed n is an interval, not the point d: n is not exactly
//   normal (for a sliver the rounding of the cross product turns it by an angle of order eps E / |n|, E =
//   |e0|_inf |e1|_inf).  No bound on that angle is needed: the other two corners are projected too, and
//   spread covers the interval as computed, so step 4 is step 3 on the axis n with d - spread <= every p_k
//   <= d + spread.  The projection errors are step 3's, the rounding of q - d and of the two sums of t add
//   eps |n|_1 (2 Wv + Wh + 2 Wv) at most; 16 eps |n|_1 (M + W) is more than twice the total.  For a sliver or
//   a segment n is rounding noise, spread is as large as |d| and step 4 rejects little: steps 1 and 3 are
//   the whole test for a segment.
// The false positives the slacks admit are MEASURED, not derived (the axes a and n are perturbed ones): over
// tests/test_overlap_cpu.py's pairs no accepted pair is separated from the box grown by g eps M on every
// side with g = kOverlapG below; the test pins 4 g.  The kernel uses nothing from g.
//
// boxPlane(normal, point, mn, mx): validity (normal, point and bounds finite, mn <= mx), c and h as above,
//   t = normal . (c - point), r = h . |normal|, slack = (8 eps |normal|_1) ((M + D) + Wh) with M over the
//   bounds and the point, D the largest |c - point| component, Wh the largest h component; true unless
//   |t| > r + slack.  (First-order need eps |normal|_1 (M + 4 D + 4 Wh), by the argument of step 3.)
// boxSphere(centre, sqRadius, mn, mx), the sphere's SURFACE as pointSphere means it: validity (sqRadius
//   finite and >= 0 too), dmin2 = boxDist2 (mrt_nearest.hpp), dmax2 = (fx fx + fy fy) + fz fz with f_a =
//   max(|centre.a - mn.a|, |mx.a - centre.a|), the farthest corner; true unless dmin2 > sqRadius (1 + kappa)
//   or dmax2 < sqRadius (1 - kappa), kappa = 2^-21 = 8 eps.  The inputs are floats, so each difference has one
//   relative rounding, each square one more and the two sums two: dmin2 and dmax2 are within (1 + eps)^5 of
//   their exact values, and the product with (1 +- kappa) adds one; 8 eps covers the six.
// An area light goes through boxTriangle on its A, AB, AC.
//
// The walk (overlapBox): planes, spheres and area lights one by one, then the triangles - under BVH a
// depth-first descent of the reference tree (triNodes / triRootRef; both children overlapping: the right
// one pushed, the left one entered), under Naive the input-order loop.
//
// The cull is exact and needs no certified bound: a node is skipped only when node.mn.a > q.mx.a or
// node.mx.a < q.mn.a on some axis, strict and false for NaN - step 1's compare on a box that contains the
// triangle's own hull.  What the builder gives (mrt_scene.cpp; triNodes holds these floats unquantized):
//   - aabbOf forms the hull with vmin / vmax, that is stdmin / stdmax, which return their first argument
//     unless the second compares strictly below / above it.  A triangle's bound is therefore NaN only where
//     the corner A itself is; an infinite corner gives an infinite bound, and such a triangle is never
//     accepted (step 0).
//   - a node's box accumulates surrounding(next, acc) over its triangles in order.  Over bounds that are not
//     NaN (infinities included) it is their true minimum and maximum, so it contains the hull of every
//     finite triangle below the node.
//   - a NaN bound (a NaN first corner) turns acc into NaN, and a NaN acc is REPLACED by the next bound:
//     stdmin(next, NaN) is next.  So a node's bound is not "NaN from the first NaN on": the triangles before
//     a NaN-cornered one in the same node may lie outside its stored box.  Where a scene holds a triangle
//     whose first corner has a NaN coordinate, the BVH walk may skip finite triangles that Naive finds; every
//     other scene - infinite and overflowing coordinates included - has BVH, Naive and the host agree.
//
// Cost.  With only `any` wanted (kAny) the walk stops at a lane's first acceptance and keeps no list: the
// occupancy test.  Otherwise every accepted candidate is met - the K smallest input indices cannot be known
// otherwise - so a box that contains the scene costs what Naive costs.  That is allowed.
#pragma once

#include "mrt_nearest.hpp"

namespace mrt {

constexpr float kOverlapEps8 = 4.76837158203125e-07F;  // 8 eps = 2^-21: the slacks' factor, and boxSphere's kappa
constexpr float kOverlapG = 64.0F;                      // the measured false-positive growth, in eps M (see above)
constexpr int kOverlapThreads = 64;  // one wave per workgroup: 4 KB of stack + 4 B x K x 64 of list

MRT_HD bool finiteF(float x) { return fabsf(x) <= 3.4028234663852886e+38F; }  // (false for NaN)
MRT_HD bool finite3(v3 a) { return finiteF(a.x) && finiteF(a.y) && finiteF(a.z); }
MRT_HD v3 vabs(v3 a) { return v3{fabsf(a.x), fabsf(a.y), fabsf(a.z)}; }
MRT_HD float norm1(v3 a) { return (fabsf(a.x) + fabsf(a.y)) + fabsf(a.z); }
MRT_HD float normInf(v3 a) { return stdmax(stdmax(fabsf(a.x), fabsf(a.y)), fabsf(a.z)); }
// finite bounds with mn <= mx on every axis
MRT_HD bool boxValid(v3 mn, v3 mx) {
    return finite3(mn) && finite3(mx) && !(mn.x > mx.x) && !(mn.y > mx.y) && !(mn.z > mx.z);
}
// step 1's compare, for a hull or a tree node: true where the two boxes are apart on some axis (strict, false
// for NaN)
MRT_HD bool boxesApart(float amnx, float amny, float amnz, float amxx, float amxy, float amxz, v3 mn, v3 mx) {
    return amnx > mx.x || amxx < mn.x || amny > mx.y || amxy < mn.y || amnz > mx.z || amxz < mn.z;
}

// step 3 for one axis: mw = M + W
MRT_HD bool crossAxisApart(v3 a, v3 v0, v3 v1, v3 v2, v3 h, float mw) {
    const float p0 = dot(a, v0), p1 = dot(a, v1), p2 = dot(a, v2);
    const float r = dot(h, vabs(a));
    const float t = r + (kOverlapEps8 * norm1(a)) * mw;
    return (p0 > t && p1 > t && p2 > t) || (p0 < -t && p1 < -t && p2 < -t);
}

MRT_HD bool boxTriangle(v3 A, v3 AB, v3 AC, v3 mn, v3 mx) {
    const v3 P0 = A, P1 = A + AB, P2 = A + AC;
    if (!finite3(P0) || !finite3(P1) || !finite3(P2) || !boxValid(mn, mx)) return false;
    const v3 lo = vmin(P0, vmin(P1, P2)), hi = vmax(P0, vmax(P1, P2));
    if (boxesApart(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, mn, mx)) return false;
    const v3 c = mn * 0.5F + mx * 0.5F, h = mx * 0.5F - mn * 0.5F;
    const v3 v0 = P0 - c, v1 = P1 - c, v2 = P2 - c;
    const v3 e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2;
    const float M = stdmax(stdmax(normInf(lo), normInf(hi)), stdmax(normInf(mn), normInf(mx)));
    const float W = stdmax(stdmax(normInf(v0), normInf(v1)), normInf(v2)) + normInf(h);
    const float mw = M + W;
    const v3 e[3] = {e0, e1, e2};
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (crossAxisApart(v3{0.0F, -e[j].z, e[j].y}, v0, v1, v2, h, mw)) return false;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (crossAxisApart(v3{e[j].z, 0.0F, -e[j].x}, v0, v1, v2, h, mw)) return false;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (crossAxisApart(v3{-e[j].y, e[j].x, 0.0F}, v0, v1, v2, h, mw)) return false;
    const v3 n = cross(e0, e1);
    const float d = dot(n, v0);
    const float r = dot(h, vabs(n));
    const float spread = stdmax(fabsf(dot(n, v1) - d), fabsf(dot(n, v2) - d));
    const float t = r + (spread + ((2.0F * kOverlapEps8) * norm1(n)) * mw);
    return !(d > t || d < -t);
}

MRT_HD bool boxPlane(v3 normal, v3 point, v3 mn, v3 mx) {
    if (!finite3(normal) || !finite3(point) || !boxValid(mn, mx)) return false;
    const v3 c = mn * 0.5F + mx * 0.5F, h = mx * 0.5F - mn * 0.5F;
    const v3 cp = c - point;
    const float t = dot(normal, cp);
    const float r = dot(h, vabs(normal));
    const float M = stdmax(stdmax(normInf(mn), normInf(mx)), normInf(point));
    const float slack = (kOverlapEps8 * norm1(normal)) * ((M + normInf(cp)) + normInf(h));
    return !(fabsf(t) > r + slack);
}

MRT_HD bool boxSphere(v3 centre, float sqRadius, v3 mn, v3 mx) {
    if (!finite3(centre) || !finiteF(sqRadius) || sqRadius < 0.0F || !boxValid(mn, mx)) return false;
    const float dmin2 = boxDist2(mn.x, mn.y, mn.z, mx.x, mx.y, mx.z, centre);
    const float fx = stdmax(fabsf(centre.x - mn.x), fabsf(mx.x - centre.x));
    const float fy = stdmax(fabsf(centre.y - mn.y), fabsf(mx.y - centre.y));
    const float fz = stdmax(fabsf(centre.z - mn.z), fabsf(mx.z - centre.z));
    const float dmax2 = (fx * fx + fy * fy) + fz * fz;
    return !(dmin2 > sqRadius * (1.0F + kOverlapEps8) || dmax2 < sqRadius * (1.0F - kOverlapEps8));
}

// mrt_box_overlap / mrt_kat_box_overlap: pair i of a kind (mrt_point_distance's kinds and layouts) against
// the box (mn xyz, mx xyz) at b
MRT_HD bool overlapPrim(int kind, const float* f, const float* b) {
    const v3 mn{b[0], b[1], b[2]}, mx{b[3], b[4], b[5]};
    if (kind == 1) return boxPlane(v3{f[0], f[1], f[2]}, v3{f[3], f[4], f[5]}, mn, mx);
    if (kind == 2) return boxSphere(v3{f[0], f[1], f[2]}, f[3], mn, mx);
    return boxTriangle(v3{f[0], f[1], f[2]}, v3{f[3], f[4], f[5]}, v3{f[6], f[7], f[8]}, mn, mx);
}

// What one lane holds.  The list (kAny false): one dword per entry, kind << 28 | INPUT index, so that integer
// order is the list's order (kind, then input index); in LDS, laid out [k][thread], kept sorted by insertion.
// Candidates arrive in walk order, so a full list still takes a candidate below its last entry, and only
// counts the others.  K may be 0 (count only: nothing is held).  kAny: no list, the first acceptance ends
// the walk.
template <bool kAny>
struct OverlapHeld {
    uint32_t* code;  // &array[threadIdx.x]; entry k at [k * kOverlapThreads] (kAny: not read)
    int K;           // entries wanted (at most the array's ceiling)
    int n;           // entries held: min(count, K)
    int count;       // accepted candidates, held or not (kAny: 0 or 1)
    int tests;       // overlap-function evaluations
    __device__ __forceinline__ void reset() {
        n = 0;
        count = 0;
        tests = 0;
    }
    __device__ __forceinline__ void accept(uint32_t cc) {
        ++count;
        if (kAny || K == 0) return;
        if (n == K && !(cc < code[(K - 1) * kOverlapThreads])) return;
        int k = n < K ? n++ : K - 1;  // the slot that opens: a new last one, or the last entry's (it drops out)
        for (; k > 0; --k) {
            const uint32_t pc = code[(k - 1) * kOverlapThreads];
            if (pc < cc) break;
            code[k * kOverlapThreads] = pc;
        }
        code[k * kOverlapThreads] = cc;
    }
};

// One triangle (BVH-order index j); its input index costs one triOrder load, and only when it is accepted.
template <bool kAny>
__device__ __forceinline__ void overlapTriangle(const DScene& s, const QueryTables& tb, int j, v3 mn, v3 mx,
                                                OverlapHeld<kAny>& ol) {
    const float4* g = s.triGeom + 3 * j;
    ++ol.tests;
    if (boxTriangle(xyz(ld4(g)), xyz(ld4(g + 1)), xyz(ld4(g + 2)), mn, mx))
        ol.accept(kAny ? 0u : encodePrim(kTriangle, static_cast<uint32_t>(tb.triOrder[j])));
}

// The reference tree, depth first (multiTraverse's loop with the box compare for the slab test).
template <bool kAny, class Stack>
__device__ __forceinline__ void overlapTriangles(const DScene& s, const QueryTables& tb, v3 mn, v3 mx,
                                                 OverlapHeld<kAny>& ol, Stack& st) {
    const GRoot& root = s.triRootRef;
    if (root.count == 0) return;
    if (boxesApart(root.bmin[0], root.bmin[1], root.bmin[2], root.bmax[0], root.bmax[1], root.bmax[2], mn, mx)) return;
    const int base = st.sp;
    int ref = root.ref;
    while (true) {
        if (ref >= 0) {
            const float4* np = reinterpret_cast<const float4*>(s.triNodes + ref);
            const float4 n0 = np[0], n1 = np[1], n2 = np[2];
            const int4 n3 = reinterpret_cast<const int4*>(np)[3];
            const bool goL = !boxesApart(n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, mn, mx);
            const bool goR = !boxesApart(n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, mn, mx);
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
                overlapTriangle(s, tb, first + k, mn, mx, ol);
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

// The accepted set of one box into ol (reset by the caller).  One block per kind, each reading through its own
// base pointer (mrt_neighbours.hpp records why).  An invalid box accepts nothing and costs no evaluation.
template <bool kAny, class Stack>
__device__ __forceinline__ void overlapBox(const DScene& s, const QueryTables& tb, v3 mn, v3 mx, OverlapHeld<kAny>& ol,
                                           Stack& st) {
    if (!boxValid(mn, mx)) return;
    const bool accel = s.accel == kAccBVH || s.accel == kAccNaive;  // else the lights only
    if (accel) {
        for (int j = 0; j < s.planeRoot.count; ++j) {
            ++ol.tests;
            if (boxPlane(xyz(s.planes[2 * j]), xyz(s.planes[2 * j + 1]), mn, mx)) {
                ol.accept(kAny ? 0u : encodePrim(kPlane, static_cast<uint32_t>(tb.planeOrder[j])));
                if (kAny) return;
            }
        }
        for (int j = 0; j < s.sphereRoot.count; ++j) {
            const float4 c4 = s.spheres[2 * j];
            ++ol.tests;
            if (boxSphere(xyz(c4), c4.w, mn, mx)) {
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
        if (boxTriangle(xyz(a4), xyz(l[1]), xyz(l[2]), mn, mx)) {
            ol.accept(encodePrim(kLight, static_cast<uint32_t>(j)));
            if (kAny) return;
        }
    }
    if (s.accel == kAccBVH) {
        overlapTriangles(s, tb, mn, mx, ol, st);
    } else if (s.accel == kAccNaive) {
        for (int i = 0; i < s.triRoot.count; ++i) {
            overlapTriangle(s, tb, s.triNaive[i], mn, mx, ol);
            if (kAny && ol.count != 0) return;
        }
    }
}
}  // namespace mrt
