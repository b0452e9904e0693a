// mrt_nearest.hpp - nearest-point queries (mrt_nearest_points_device): the distance functions, shared
// by the host (mrt_point_distance) and the kernels, and the per-lane walk that minimises them.
//
// The answer for a point is DEFINED as the least, in the total order (d2, kind, input index), of the
// functions below over the candidates whose d2 is below the point's bound and not NaN.  For slivers
// pointTriangle may return a point of the triangle that is not the closest one; the definition stands.
// Every translation unit compiles with -ffp-contract=off, so host and device give the same bits.
//
// The walk (nearestPoint): planes, spheres and area lights one by one first, then the triangles - under
// BVH a descent of the reference tree (triNodes / triRootRef), near child first by box distance, the far
// child pushed with its box distance and tested again when popped; under Naive a loop in input order.
//
// The cull.  boxDist2 is lb = dx*dx + dy*dy + dz*dz with d = max(0, mn - p, p - mx) per axis.  Rounding is
// monotone, so an ancestor's lb is never above the lb of a box inside it, and every reference box above
// a triangle contains the hull of its corners A, fl(A + AB), fl(A + AC) (aabbOf).  After pointTriangle's
// clamp q is a convex combination of those corners up to a few roundings of size eps * M (eps = 2^-24,
// M the largest |coordinate| of p and the box), so with c = k * eps * M
//     d2 >= lb - c * sqrt(lb) - c^2                                  (the lemma; k = kNearestK = 32,
// four times the bound tests/test_nearest_cpu.py holds the real function to).  f(s) = s^2 - c s - c^2
// grows for s > c / 2, and f(sb + 2c) = sb^2 + 3 sb c + c^2 >= sb^2; so sqrt(lb) > sqrt(best) + 2c gives
// d2 > best: no triangle in the box wins or ties.  thr = (sqrtf(best) + 2 c1)^2 * (1 + 2^-20), with
// c1 = k * eps * Mq and Mq the largest |coordinate| of p and the root box (>= every M, a NaN kept);
// the 2^-20 covers the three roundings of thr.  A box is skipped only when lb > thr: strict, false for
// NaN (a non-finite box, Mq or best never culls), and thr is +inf while best is.
#pragma once

#include "mrt_kernels.hpp"

namespace mrt {

struct PointDist {
    float d2;  // squared distance
    v3 q;      // the nearest point
    float u, v;  // triangle: the weights of B and C (q = (A + AB * u) + AC * v); else 0, 0
};

// Ericson's closest point on a triangle (Real-Time Collision Detection 5.1.5), A, AB, AC as triGeom holds
// them.  Order of operations, every dot as mrt::dot ((x + y) + z):
//   ap = p - A; d1 = AB.ap; d2 = AC.ap;            bp = ap - AB; d3 = AB.bp; d4 = AC.bp;
//   cp = ap - AC; d5 = AB.cp; d6 = AC.cp;          vc = d1*d4 - d3*d2; vb = d5*d2 - d1*d6; va = d3*d6 - d5*d4;
// regions in this order, (v, w) the weights of B and C:
//   A:  d1 <= 0 && d2 <= 0                          -> (0, 0)
//   B:  d3 >= 0 && d4 <= d3                         -> (1, 0)
//   AB: vc <= 0 && d1 >= 0 && d3 <= 0               -> (d1 / (d1 - d3), 0)
//   C:  d6 >= 0 && d5 <= d6                         -> (0, 1)
//   AC: vb <= 0 && d2 >= 0 && d6 <= 0               -> (0, d2 / (d2 - d6))
//   BC: va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0     -> w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w
//   face (the fall-through)                         -> den = 1 / ((va + vb) + vc); v = vb * den; w = vc * den
// then always v = fminf(fmaxf(v, 0), 1); w = fminf(fmaxf(w, 0), 1 - v) (NaN -> 0: the function is total
// and q stays on the triangle), q = (A + AB * v) + AC * w, e = p - q, d2 = (e.x*e.x + e.y*e.y) + e.z*e.z.
MRT_HD PointDist pointTriangle(v3 A, v3 AB, v3 AC, v3 p) {
    const v3 ap = p - A;
    const float d1 = dot(AB, ap), d2 = dot(AC, ap);
    const v3 bp = ap - AB;
    const float d3 = dot(AB, bp), d4 = dot(AC, bp);
    const v3 cp = ap - AC;
    const float d5 = dot(AB, cp), d6 = dot(AC, cp);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    float v, w;
    if (d1 <= 0.0F && d2 <= 0.0F) {
        v = 0.0F;
        w = 0.0F;
    } else if (d3 >= 0.0F && d4 <= d3) {
        v = 1.0F;
        w = 0.0F;
    } else if (vc <= 0.0F && d1 >= 0.0F && d3 <= 0.0F) {
        v = d1 / (d1 - d3);
        w = 0.0F;
    } else if (d6 >= 0.0F && d5 <= d6) {
        v = 0.0F;
        w = 1.0F;
    } else if (vb <= 0.0F && d2 >= 0.0F && d6 <= 0.0F) {
        v = 0.0F;
        w = d2 / (d2 - d6);
    } else if (va <= 0.0F && (d4 - d3) >= 0.0F && (d5 - d6) >= 0.0F) {
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        v = 1.0F - w;
    } else {
        const float den = 1.0F / ((va + vb) + vc);
        v = vb * den;
        w = vc * den;
    }
    v = fminf(fmaxf(v, 0.0F), 1.0F);
    w = fminf(fmaxf(w, 0.0F), 1.0F - v);
    PointDist r;
    r.q = (A + AB * v) + AC * w;
    const v3 e = p - r.q;
    r.d2 = (e.x * e.x + e.y * e.y) + e.z * e.z;
    r.u = v;
    r.v = w;
    return r;
}

// normal as makePlane normalised it: s = normal.(p - point), q = p - normal * s, d2 = s * s
MRT_HD PointDist pointPlane(v3 normal, v3 point, v3 p) {
    const float s = dot(normal, p - point);
    PointDist r;
    r.q = p - normal * s;
    r.d2 = s * s;
    r.u = 0.0F;
    r.v = 0.0F;
    return r;
}

// the surface of the sphere: d = |len - r|; q = c + (p - c) * (r / len), or c + (r, 0, 0) at the centre
MRT_HD PointDist pointSphere(v3 c, float sqRadius, v3 p) {
    const v3 pc = p - c;
    const float len = sqrtf(dot(pc, pc));
    const float rad = sqrtf(sqRadius);
    const float d = fabsf(len - rad);
    PointDist r;
    r.q = len == 0.0F ? c + v3{rad, 0.0F, 0.0F} : c + pc * (rad / len);
    r.d2 = d * d;
    r.u = 0.0F;
    r.v = 0.0F;
    return r;
}

// mrt_point_distance / mrt_kat_point_distance: pair i of a kind (1 plane: normal, point; 2 sphere:
// centre, sqRadius; 3, 4 triangle: A, AB, AC) through the functions above
MRT_HD int pointPrimFloats(int kind) { return kind == 1 ? 6 : kind == 2 ? 4 : 9; }
MRT_HD PointDist pointPrim(int kind, const float* f, v3 p) {
    if (kind == 1) return pointPlane(v3{f[0], f[1], f[2]}, v3{f[3], f[4], f[5]}, p);
    if (kind == 2) return pointSphere(v3{f[0], f[1], f[2]}, f[3], p);
    return pointTriangle(v3{f[0], f[1], f[2]}, v3{f[3], f[4], f[5]}, v3{f[6], f[7], f[8]}, p);
}

constexpr float kNearestK = 32.0F;  // the lemma's k (see above; tests hold the function to k / 4)
constexpr int kNearestThreads = 64;  // one wave per workgroup: 8 stack entries of 8 B per lane = 4 KB of LDS

// max(0, mn - p, p - mx), NaN where either difference is (a NaN bound, or inf - inf)
MRT_HD float axisDist(float mn, float mx, float p) {
    const float a = mn - p, b = p - mx;
    float d = stdmax(a, b);  // a NaN a is kept, a NaN b is not
    d = b != b ? b : d;
    return d < 0.0F ? 0.0F : d;
}
// squared distance from p to the box (0 inside); NaN for a box with a NaN bound: such a box is never skipped
MRT_HD float boxDist2(float mnx, float mny, float mnz, float mxx, float mxy, float mxz, v3 p) {
    const float dx = axisDist(mnx, mxx, p.x), dy = axisDist(mny, mxy, p.y), dz = axisDist(mnz, mxz, p.z);
    return (dx * dx + dy * dy) + dz * dz;
}

// The held answer of one lane: the best candidate so far (code: BVH-order, kNoPrim none), the bound it
// must beat (d2; the point's bound2 while nothing is held) and the cull threshold derived from it.
struct NearestBest {
    float d2;
    uint32_t code;
    v3 q;
    float u, v;
    float c2;   // 2 c1 = 2 * k * eps * Mq
    float thr;  // boxes with lb > thr hold no winner
    int tests;
    __device__ __forceinline__ void setThr() {
        const float s = sqrtf(d2) + c2;
        thr = (s * s) * (1.0F + 9.5367431640625e-07F);
    }
};

// the candidate's index in input order (lights keep theirs)
__device__ __forceinline__ int32_t nearestInput(const QueryTables& tb, uint32_t code) {
    const uint32_t k = primKind(code);
    const int32_t* order = k == kTriangle ? tb.triOrder : k == kPlane ? tb.planeOrder : k == kSphere ? tb.sphereOrder : nullptr;
    const int32_t b = static_cast<int32_t>(primIndex(code));
    return order != nullptr ? order[b] : b;
}

// A candidate replaces the held one when it is smaller, or bit-equal and earlier in (kind, input index);
// a NaN d2 is never accepted (both compares are false), nor one at or above the bound while nothing is held.
__device__ __forceinline__ void nearestOffer(const QueryTables& tb, const PointDist& c, uint32_t code, NearestBest& nb) {
    ++nb.tests;
    bool take = c.d2 < nb.d2;
    if (!take && c.d2 == nb.d2 && nb.code != kNoPrim) {
        const uint32_t kc = primKind(code), kh = primKind(nb.code);
        take = kc != kh ? kc < kh : nearestInput(tb, code) < nearestInput(tb, nb.code);
    }
    if (!take) return;
    nb.d2 = c.d2;
    nb.code = code;
    nb.q = c.q;
    nb.u = c.u;
    nb.v = c.v;
    nb.setThr();
}

__device__ __forceinline__ void nearestTriangle(const DScene& s, const QueryTables& tb, int j, v3 p, uint32_t src,
                                                NearestBest& nb) {
    const uint32_t code = encodePrim(kTriangle, static_cast<uint32_t>(j));
    if (code == src) return;
    const float4* g = s.triGeom + 3 * j;
    nearestOffer(tb, pointTriangle(xyz(ld4(g)), xyz(ld4(g + 1)), xyz(ld4(g + 2)), p), code, nb);
}

// largest |x| so far, a NaN kept once met
__device__ __forceinline__ float absMaxNan(float m, float x) {
    const float a = fabsf(x);
    return (a > m || a != a) ? a : m;
}

// The reference tree, best first.  Stack: TStack (reference and box distance per entry).  Held: what the
// lane keeps (NearestBest, or mrt_neighbours.hpp's list) - its c2, thr and setThr(), and a nearestTriangle
// that offers it one triangle.
template <class Stack, class Held>
__device__ __forceinline__ void nearestTriangles(const DScene& s, const QueryTables& tb, v3 p, uint32_t src,
                                                 Held& nb, Stack& st) {
    const GRoot& root = s.triRootRef;
    if (root.count == 0) return;
    float m = fabsf(p.x);
    m = absMaxNan(m, p.y);
    m = absMaxNan(m, p.z);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        m = absMaxNan(m, root.bmin[a]);
        m = absMaxNan(m, root.bmax[a]);
    }
    nb.c2 = (2.0F * kNearestK * 5.9604644775390625e-08F) * m;
    nb.setThr();
    if (boxDist2(root.bmin[0], root.bmin[1], root.bmin[2], root.bmax[0], root.bmax[1], root.bmax[2], p) > nb.thr) return;
    const int base = st.sp;
    int ref = root.ref;
    while (true) {
        if (ref >= 0) {
            const float4* np = reinterpret_cast<const float4*>(s.triNodes + ref);
            const float4 n0 = np[0], n1 = np[1], n2 = np[2];
            const int4 n3 = reinterpret_cast<const int4*>(np)[3];
            const float ll = boxDist2(n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, p);
            const float lr = boxDist2(n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, p);
            const bool goL = !(ll > nb.thr), goR = !(lr > nb.thr);
            if (goL && goR) {
                const bool leftNear = ll <= lr;
                st.push(leftNear ? n3.y : n3.x, leftNear ? lr : ll);
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
            for (int k = 0; k < count; ++k) nearestTriangle(s, tb, first + k, p, src, nb);
        }
        bool found = false;
        while (st.sp != base) {  // the far children, against the bound as it is now
            const int2 e = st.pop();
            if (__int_as_float(e.y) > nb.thr) continue;
            ref = e.x;
            found = true;
            break;
        }
        if (!found) return;
    }
}

// The answer of one point.  bound2: the squared search radius (+inf unbounded, 0 finds nothing).
template <class Stack>
__device__ __forceinline__ NearestBest nearestPoint(const DScene& s, const QueryTables& tb, v3 p, float bound2,
                                                    uint32_t src, Stack& st) {
    NearestBest nb{bound2, kNoPrim, v3{0.0F, 0.0F, 0.0F}, 0.0F, 0.0F, 0.0F, 0.0F, 0};
    const bool accel = s.accel == kAccBVH || s.accel == kAccNaive;  // else the lights only
    if (accel) {
        for (int j = 0; j < s.planeRoot.count; ++j) {
            const uint32_t code = encodePrim(kPlane, static_cast<uint32_t>(j));
            if (code == src) continue;
            nearestOffer(tb, pointPlane(xyz(s.planes[2 * j]), xyz(s.planes[2 * j + 1]), p), code, nb);
        }
        for (int j = 0; j < s.sphereRoot.count; ++j) {
            const float4 c4 = s.spheres[2 * j];
            nearestOffer(tb, pointSphere(xyz(c4), c4.w, p), encodePrim(kSphere, static_cast<uint32_t>(j)), nb);
        }
    }
    for (int j = 0; j < s.nLights; ++j) {
        const float4* l = s.lights + 4 * j;
        const float4 a4 = l[0];
        if (__float_as_int(a4.w) != 1) continue;  // point lights are never candidates
        nearestOffer(tb, pointTriangle(xyz(a4), xyz(l[1]), xyz(l[2]), p), encodePrim(kLight, static_cast<uint32_t>(j)), nb);
    }
    if (s.accel == kAccBVH) {
        nearestTriangles(s, tb, p, src, nb, st);
    } else if (s.accel == kAccNaive) {
        for (int i = 0; i < s.triRoot.count; ++i) nearestTriangle(s, tb, s.triNaive[i], p, src, nb);
    }
    return nb;
}
}  // namespace mrt
