// mrt_multi_hit.hpp - the multi-hit walk (mrt_cast_multi_hits_device): the first K hits along a ray,
// in order, and the number of hits.
//
// A ray's hit set is every primitive Shader::rayTrace's intersection part would accept if no accepted
// hit shortened the ray: the leaf routines of mrt_device.hpp (leafPlanes / leafSpheres /
// leafTriangles, and triTest for the lights) are called one primitive at a time against a fresh Best
// whose length is the ray's own tmax, so what they accept is Plane / Sphere / Triangle::intersect's
// acceptance at that length (neither t < eps nor t >= tmax, self-exclusion included) in their own
// arithmetic.  The visit set is traverse<>'s: every leaf whose box and whose ancestors' boxes pass
// the reference slab predicate, nothing culled - a cull needs a bound that shrinks, and the list's
// bound (its K-th entry) says nothing about the count, which every accepted hit enters.
//
// Order.  traverse<> reaches leaves in ascending BVH-order index (left first, right pushed), the
// kinds are walked planes, spheres, triangles, lights (Shader.cpp:104-111), and Naive tests in input
// order.  So the order of arrival is the tie order of the closest-hit walks (betterThan: kind as
// evaluated, then the lower index), and a stable insertion by t alone gives the documented total
// order: a new hit goes behind every held hit whose t is not greater.  A NaN t is not inserted and
// not counted: an ordered list has no place for it.
#pragma once

#include "mrt_kernels.hpp"

namespace mrt {

constexpr int kMultiThreads = 64;  // one wave per workgroup: K-buffer (16 x 16 B) + stack (64 B) per lane = 20 KB at K = 16

// A lane's K-buffer over four LDS arrays laid out [k][thread]: entry k of this lane at [k * kMultiThreads],
// so the wave's accesses to one k fall on 64 consecutive dwords (conflict-free).
struct KBuffer {
    float* t;        // &array[threadIdx.x]
    uint32_t* code;  // encodePrim(kind, walk-order index)
    float* u;
    float* v;
    int K;           // entries wanted (at most the arrays' ceiling)
    int n;           // entries held: min(count, K)
    int count;       // accepted hits, held or not
    float tmax;      // the ray's interval end
    __device__ __forceinline__ void reset(float rayMax) {
        n = 0;
        count = 0;
        tmax = rayMax;
    }
    // (hits arrive in tie order: behind every held entry whose t is not greater)
    __device__ __forceinline__ void insert(const Best& b) {
        if (b.code == kNoPrim || !(b.t == b.t)) return;  // not accepted, or accepted with a NaN t
        ++count;
        if (n == K && !(b.t < t[(K - 1) * kMultiThreads])) return;  // behind the last entry of a full list
        int k = n < K ? n++ : K - 1;  // the slot that opens: a new last one, or the last entry's (it drops out)
        for (; k > 0 && t[(k - 1) * kMultiThreads] > b.t; --k) {
            t[k * kMultiThreads] = t[(k - 1) * kMultiThreads];
            code[k * kMultiThreads] = code[(k - 1) * kMultiThreads];
            u[k * kMultiThreads] = u[(k - 1) * kMultiThreads];
            v[k * kMultiThreads] = v[(k - 1) * kMultiThreads];
        }
        t[k * kMultiThreads] = b.t;
        code[k * kMultiThreads] = b.code;
        u[k * kMultiThreads] = b.u;
        v[k * kMultiThreads] = b.v;
    }
};

// One primitive (BVH-order index j) through the closest-hit walk's leaf routine against the ray's
// whole interval (kTies false: the plain `t >= length` rejection; there is no earlier hit to tie with).
template <int kKind>
__device__ __forceinline__ void multiTest(const DScene& s, int j, v3 o, v3 d, uint32_t src, KBuffer& kb) {
    Best b{kb.tmax, 0.0F, 0.0F, kNoPrim};
    uint32_t nTri = 0;
    if (kKind == kTriangle) leafTriangles<false, false>(s, j, 1, o, d, src, &b, &nTri);
    if (kKind == kPlane) leafPlanes<false, false>(s, j, 1, o, d, src, &b);
    if (kKind == kSphere) leafSpheres<false, false>(s, j, 1, o, d, &b);
    kb.insert(b);
}

// traverse<>'s loop (BVH.hpp:327-384: the same boxes in the same order, left first, right pushed)
// with every primitive of a reached leaf offered to the K-buffer; it never ends early.
template <int kKind, class Stack>
__device__ __forceinline__ void multiTraverse(const DScene& s, const GNode* nodes, const GRoot& root, v3 o, v3 d, v3 inv,
                                              uint32_t src, KBuffer& kb, Stack& st) {
    if (root.count == 0) return;  // BVH.hpp:328-330
    float te;
    if (!slab(root.bmin[0], root.bmin[1], root.bmin[2], root.bmax[0], root.bmax[1], root.bmax[2], o, inv, &te)) return;
    const int base = st.sp;
    int ref = root.ref;
    while (true) {
        if (ref >= 0) {
            const float4* np = reinterpret_cast<const float4*>(nodes + ref);
            const float4 n0 = np[0], n1 = np[1], n2 = np[2];
            const int4 n3 = reinterpret_cast<const int4*>(np)[3];
            float tl, tr;
            const bool hl = slab(n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, o, inv, &tl);
            const bool hr = slab(n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, o, inv, &tr);
            if (hl && hr) {
                st.push(n3.y, tr);
                ref = n3.x;
                continue;
            }
            if (hl) {
                ref = n3.x;
                continue;
            }
            if (hr) {
                ref = n3.y;
                continue;
            }
        } else {
            const int first = leafFirst(ref), count = leafCount(ref);
            for (int k = 0; k < count; ++k) multiTest<kKind>(s, first + k, o, d, src, kb);
        }
        if (st.sp == base) return;
        ref = st.pop().x;
    }
}

// The hit set of one ray into kb (reset by the caller): the accelerator's primitives, then the area
// lights (Shader.cpp:166-171, as closestHit tests them).  An accelerator id that builds nothing leaves
// the lights only; the RegularGrid is refused before any launch.
template <class Stack>
__device__ __forceinline__ void multiHits(const DScene& s, v3 o, v3 d, uint32_t src, KBuffer& kb, Stack& st) {
    if (s.accel == kAccBVH) {
        const v3 inv = v3{1.0F / d.x, 1.0F / d.y, 1.0F / d.z};
        multiTraverse<kPlane>(s, s.planeNodes, s.planeRoot, o, d, inv, src, kb, st);
        multiTraverse<kSphere>(s, s.sphereNodes, s.sphereRoot, o, d, inv, src, kb, st);
        multiTraverse<kTriangle>(s, s.triNodes, s.triRootRef, o, d, inv, src, kb, st);
    } else if (s.accel == kAccNaive) {  // naiveWalk's loops: every primitive in input order
        for (int i = 0; i < s.planeRoot.count; ++i) multiTest<kPlane>(s, s.planeNaive[i], o, d, src, kb);
        for (int i = 0; i < s.sphereRoot.count; ++i) multiTest<kSphere>(s, s.sphereNaive[i], o, d, src, kb);
        for (int i = 0; i < s.triRoot.count; ++i) multiTest<kTriangle>(s, s.triNaive[i], o, d, src, kb);
    }
    for (int j = 0; j < s.nLights; ++j) {
        const float4* l = s.lights + 4 * j;
        const float4 a4 = l[0];
        if (__float_as_int(a4.w) != 1) continue;  // point lights are never hit
        float t, u, v;
        if (!triTest(a4, l[1], l[2], o, d, &t, &u, &v)) continue;
        if (t < kEpsilon || t >= kb.tmax) continue;  // Triangle.cpp:104
        kb.insert(Best{t, u, v, encodePrim(kLight, static_cast<uint32_t>(j))});
    }
}

}  // namespace mrt
