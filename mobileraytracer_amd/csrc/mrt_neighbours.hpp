// mrt_neighbours.hpp - neighbour queries (mrt_neighbours_device): the K nearest surfaces to a point, in
// order, and the number of surfaces within the point's radius.  It is to the nearest-point query
// (mrt_nearest.hpp) what the multi-hit walk is to the closest-hit walk: the same candidates, distance
// functions, acceptance (d2 < bound2, not NaN) and total order (d2, kind, input index), the same walk -
// planes, spheres and area lights one by one, then the reference tree best first (nearestTriangles) or the
// input-order loop - with a list where that walk holds one answer.
//
// The list.  One per lane, in LDS, laid out [k][thread] like the multi-hit K-buffer, and holding the two
// dwords the order needs: d2 and the BVH-order code.  q, u and v are not held: the distance functions are
// pure, so when a point is done they are evaluated once more for the held entries and give
// mrt_point_distance's bits; an insertion then moves two dwords per entry.  Candidates arrive best first
// by box, not in tie order, so the insertion compares the whole key; the codes are mapped to input order
// (QueryTables) only where two d2 are bit-equal.
//
// The cull is the nearest-point walk's certified one (lb > thr, strict, false for NaN; thr = (sqrt(b) +
// 2 c1)^2 (1 + 2^-20), mrt_nearest.hpp), and what differs is b:
//   count wanted (kCount):  b = bound2, for the whole walk.  The lemma gives d2 > bound2 for every triangle
//       of a skipped box: none of them is accepted, so none is missing from the count.  Every accepted
//       candidate is met, whether or not it enters the list; with no radius nothing is skipped.
//   count not wanted:       b = bound2 until the list is full, then its K-th d2 (below bound2: it was
//       accepted), recomputed whenever an insertion changes that entry.  The lemma gives d2 > the K-th d2
//       for every triangle of a skipped box: none of them enters the list.  A candidate bit-equal to the
//       K-th entry and earlier in the order must still displace it, and is never skipped: the lemma is
//       strict (d2 > b, not >=), so a box holding a triangle with d2 == b has lb <= thr.
#pragma once

#include "mrt_nearest.hpp"

namespace mrt {

constexpr int kNeighbourThreads = kNearestThreads;  // one wave per workgroup: 4 KB of stack + 8 B x K x 64 of list

// true where candidate a comes before b among candidates of bit-equal d2: kind, then the input index
__device__ __forceinline__ bool neighbourBefore(const QueryTables& tb, uint32_t a, uint32_t b) {
    const uint32_t ka = primKind(a), kb = primKind(b);
    return ka != kb ? ka < kb : nearestInput(tb, a) < nearestInput(tb, b);
}

template <bool kCount>
struct NeighbourList {
    float* d2;       // &array[threadIdx.x]; entry k at [k * kNeighbourThreads]
    uint32_t* code;  // encodePrim(kind, BVH-order index)
    int K;           // entries wanted (at most the arrays' ceiling)
    int n;           // entries held: min(count, K)
    int count;       // accepted candidates, held or not
    int tests;       // distance-function evaluations
    float bound2;    // the point's acceptance bound
    float cull2;     // what thr derives from: bound2, or the K-th d2 of a full list (kCount false)
    float c2;        // 2 c1 = 2 * k * eps * Mq (nearestTriangles sets it)
    float thr;       // boxes with lb > thr hold nothing wanted
    __device__ __forceinline__ void reset(float b2) {
        n = 0;
        count = 0;
        tests = 0;
        bound2 = b2;
        cull2 = b2;
        c2 = 0.0F;
        thr = 0.0F;
    }
    __device__ __forceinline__ void setThr() {
        const float s = sqrtf(cull2) + c2;
        thr = (s * s) * (1.0F + 9.5367431640625e-07F);
    }
    // One evaluated candidate.  A NaN d2 is neither counted nor inserted (the compare is false).
    __device__ __forceinline__ void offer(const QueryTables& tb, float c, uint32_t cc) {
        ++tests;
        if (!(c < bound2)) return;
        ++count;
        if (n == K) {  // a full list: only what comes before its last entry enters
            const float last = d2[(K - 1) * kNeighbourThreads];
            if (!(c < last) && !(c == last && neighbourBefore(tb, cc, code[(K - 1) * kNeighbourThreads]))) return;
        }
        int k = n < K ? n++ : K - 1;  // the slot that opens: a new last one, or the last entry's (it drops out)
        for (; k > 0; --k) {
            const float pd = d2[(k - 1) * kNeighbourThreads];
            const uint32_t pc = code[(k - 1) * kNeighbourThreads];
            if (pd < c || (pd == c && !neighbourBefore(tb, cc, pc))) break;
            d2[k * kNeighbourThreads] = pd;
            code[k * kNeighbourThreads] = pc;
        }
        d2[k * kNeighbourThreads] = c;
        code[k * kNeighbourThreads] = cc;
        if (!kCount && n == K) {  // the K-nearest search: the bound is the list's last entry from here on
            // (an equal-d2 candidate earlier in the order still gets here: see the top of this file)
            cull2 = d2[(K - 1) * kNeighbourThreads];
            setThr();
        }
    }
};

// nearestTriangles' leaf routine for a list
template <bool kCount>
__device__ __forceinline__ void nearestTriangle(const DScene& s, const QueryTables& tb, int j, v3 p, uint32_t src,
                                                NeighbourList<kCount>& nl) {
    const uint32_t code = encodePrim(kTriangle, static_cast<uint32_t>(j));
    if (code == src) return;
    const float4* g = s.triGeom + 3 * j;
    nl.offer(tb, pointTriangle(xyz(ld4(g)), xyz(ld4(g + 1)), xyz(ld4(g + 2)), p).d2, code);
}

// The distance function of a held candidate once more: the bits the walk saw (and mrt_point_distance gives).
// One block per kind, each reading through its own base pointer: with the triangles and the lights sharing
// one pointTriangle call through a pointer selected per lane (k == kLight ? lights : triGeom), hipcc's code
// for gfx950 gave the triangle lanes the lights' base (seen in the assembly and in the results).
__device__ __forceinline__ PointDist neighbourEval(const DScene& s, uint32_t code, v3 p) {
    const uint32_t k = primKind(code);
    const int j = static_cast<int>(primIndex(code));
    PointDist r{0.0F, v3{0.0F, 0.0F, 0.0F}, 0.0F, 0.0F};
    if (k == kPlane) r = pointPlane(xyz(s.planes[2 * j]), xyz(s.planes[2 * j + 1]), p);
    if (k == kSphere) {
        const float4 c4 = s.spheres[2 * j];
        r = pointSphere(xyz(c4), c4.w, p);
    }
    if (k == kTriangle) {
        const float4* g = s.triGeom + 3 * j;
        r = pointTriangle(xyz(ld4(g)), xyz(ld4(g + 1)), xyz(ld4(g + 2)), p);
    }
    if (k == kLight) {
        const float4* l = s.lights + 4 * j;
        r = pointTriangle(xyz(l[0]), xyz(l[1]), xyz(l[2]), p);
    }
    return r;
}

// The accepted set of one point into nl (reset by the caller), in nearestPoint's order of work.
template <bool kCount, class Stack>
__device__ __forceinline__ void neighbourPoint(const DScene& s, const QueryTables& tb, v3 p, uint32_t src,
                                               NeighbourList<kCount>& nl, Stack& st) {
    const bool accel = s.accel == kAccBVH || s.accel == kAccNaive;  // else the lights only
    if (accel) {
        for (int j = 0; j < s.planeRoot.count; ++j) {
            const uint32_t code = encodePrim(kPlane, static_cast<uint32_t>(j));
            if (code == src) continue;
            nl.offer(tb, pointPlane(xyz(s.planes[2 * j]), xyz(s.planes[2 * j + 1]), p).d2, code);
        }
        for (int j = 0; j < s.sphereRoot.count; ++j) {
            const float4 c4 = s.spheres[2 * j];
            nl.offer(tb, pointSphere(xyz(c4), c4.w, p).d2, encodePrim(kSphere, static_cast<uint32_t>(j)));
        }
    }
    for (int j = 0; j < s.nLights; ++j) {
        const float4* l = s.lights + 4 * j;
        const float4 a4 = l[0];
        if (__float_as_int(a4.w) != 1) continue;  // point lights are never candidates
        nl.offer(tb, pointTriangle(xyz(a4), xyz(l[1]), xyz(l[2]), p).d2, encodePrim(kLight, static_cast<uint32_t>(j)));
    }
    if (s.accel == kAccBVH) {
        nearestTriangles(s, tb, p, src, nl, st);
    } else if (s.accel == kAccNaive) {
        for (int i = 0; i < s.triRoot.count; ++i) nearestTriangle(s, tb, s.triNaive[i], p, src, nl);
    }
}

}  // namespace mrt
