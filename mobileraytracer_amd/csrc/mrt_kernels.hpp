// mrt_kernels.hpp - queue layouts, kernel argument blocks and launch wrappers.
#pragma once

#include "mrt_device.hpp"

namespace mrt {

constexpr int kShaderWhitted = 1;     // C_wrapper.cpp:155-160
constexpr int kShaderPathTracer = 2;  // C_wrapper.cpp:162-172
constexpr int kShaderDepthMap = 3;    // C_wrapper.cpp:175-179
constexpr int kShaderDiffuse = 4;     // C_wrapper.cpp:181-186 (DiffuseMaterial)
constexpr int kShaderNoShadows = 5;   // C_wrapper.cpp:188-193 (the switch's default: 0, 5, ...)
constexpr int kMaxLevels = 16;           // max ray depth + 2
constexpr int kTraceVariants = 2;        // 0: per-wave reference walk, 1: persistent while-while walk
constexpr int kDefaultTraceVariant = 1;
constexpr int kAccNaive = 1;  // Shader::Accelerator (Shader.hpp:20-24)
constexpr int kAccGrid = 2;
constexpr int kAccBVH = 3;
constexpr int kTopNodesMax = 64 * 4 / kWalkWidth;  // walk-tree nodes numbered breadth-first (4 KB staged in LDS by the walk)

// Queue segments (round 6).  Every queue a level's shading fills - the next level's rays, this level's
// shadow rays - is kQueueSegs segments of segCap / shadowSegCap slots (Level), each with its own
// counter pair on its own 256-B line: workgroup b allocates in segment b % kQueueSegs.  One counter
// for the whole queue made every allocation a same-address atomic, which queue at the memory side
// (a second such atomic per allocation cost +8.1 ms per C4 frame, spread over 8 lines +0.03 ms:
// profiles/r06_alloc_atomic_probe.txt).  A segment's rays are [g * segCap, g * segCap + count_g);
// consumers walk the segments (LevelQueue's cursors) or map a dense index over them (SegMap).
// Level 1 is one dense range [0, n) cut into segments of segCap (denseCounts).
#ifndef MRT_QUEUE_SEGS
#define MRT_QUEUE_SEGS 8
#endif
constexpr int kQueueSegs = MRT_QUEUE_SEGS;
// Device counters (ints).  Segment g's pair l = {rays of level l+1, shadow rays of level l} sits on
// two adjacent ints so k_shade allocates both with one 64-bit atomic per workgroup iteration.
constexpr int kCntSegStride = 64;                     // ints between segments' pair tables (>= 2 * (kMaxLevels + 1))
constexpr int kCntPairs = 0;                          // kQueueSegs tables
constexpr int kCntOverflow = kQueueSegs * kCntSegStride;
constexpr int kPacketStack = 128;  // the packet walk's wave-uniform stack entries (mrt_trace_packet.hpp)
#ifndef MRT_WALK_CURSORS
#define MRT_WALK_CURSORS 8
#endif
constexpr int kMaxFetchShards = MRT_WALK_CURSORS;     // work cursors per level (a multiple of the 8 XCD groups)
constexpr int kFetchStride = 32;                      // ints between cursors (a 128-byte line each)
constexpr int kCntFetchShards = kCntOverflow + kFetchStride;  // 2 kinds x kMaxLevels x kMaxFetchShards lines
constexpr int kNumCounters = kCntFetchShards + 2 * kMaxLevels * kMaxFetchShards * kFetchStride;
MRT_HD constexpr int cntRays(int level, int seg = 0) { return kCntPairs + seg * kCntSegStride + 2 * (level - 1); }
MRT_HD constexpr int cntShadows(int level, int seg = 0) { return kCntPairs + seg * kCntSegStride + 2 * level + 1; }
static_assert(kQueueSegs >= 1 && kQueueSegs <= kMaxFetchShards, "queue segments: one work cursor each at most");
static_assert(cntShadows(kMaxLevels) < kCntSegStride, "a segment's pairs within its line");

// 64-bit statistics accumulated on the device across a frame
constexpr int kStatRays = 0;        // rays of every level (camera + diffuse + specular + transmission)
constexpr int kStatShadowRays = 1;  // shadow rays
constexpr int kStatPrimary = 2;
constexpr int kStatNodes = 3;       // closest-hit kernel: child node records fetched (counting pass only)
constexpr int kStatTris = 4;        // closest-hit kernel: triangle tests (counting pass only)
constexpr int kStatOverflow = 5;
constexpr int kStatNodesShadow = 6; // any-hit kernel: child node records fetched (counting pass only)
constexpr int kStatTrisShadow = 7;  // any-hit kernel: triangle tests (counting pass only)
constexpr int kStatLevelRays = 8;                     // + level - 1: rays of each level
constexpr int kStatLevelShadows = 8 + kMaxLevels;     // + level - 1: shadow rays of each level
constexpr int kStatMaxNodesRay = 8 + 2 * kMaxLevels;  // counting builds: most node records of one ray
constexpr int kStatSkipped = kStatMaxNodesRay + 1;   // rays of a last level whose walk was skipped
constexpr int kStatShaded = kStatSkipped + 1;        // counting pass: vertices k_shade shaded (hit, not emissive, not capped)
constexpr int kStatShadeLaunches = kStatShaded + 1;  // k_shade launches of the frame
constexpr int kStatLeaves = kStatShadeLaunches + 1;  // counting pass: leaf records fetched, closest hit
constexpr int kStatLeavesShadow = kStatLeaves + 1;   // ... and any hit
// counting pass, closest hit, per level (+ level - 1): child records, triangle tests, leaf records
constexpr int kStatLevelNodes = kStatLeavesShadow + 1;
constexpr int kStatLevelTris = kStatLevelNodes + kMaxLevels;
constexpr int kStatLevelLeaves = kStatLevelTris + kMaxLevels;
constexpr int kStatLevelShaded = kStatLevelLeaves + kMaxLevels;  // counting pass: kStatShaded per level
constexpr int kStatOccluded = kStatLevelShaded + kMaxLevels;  // counting pass: occluded shadow rays
constexpr int kStatPhases = kStatOccluded + 1;  // counting pass: 2 walks x {inner, leaf, triangle} x {iterations, lanes},
                                                // then 2 walks x inner {idle, done} lanes
// counting pass, the level-1 packet walk, per wave (scalar loads: each record fetched once for the
// wave's rays): inner nodes visited, leaf records loaded, triangle records loaded
constexpr int kStatPacket = kStatPhases + 16;
// What the pass asked of its queues (k_tally; + level - 1), the largest over the pass's chunks: the
// largest count one segment of the level's ray / shadow queue was asked for, and the level's total.
// The allocation counters run past a full segment (only the writes are dropped), so after an
// overflow these are the demand the next queue plan is sized from (mrt_queue_plan.hpp): exact up to
// the first overflowed level (kStatOverflow: bit l = level l's ray or shadow queue dropped a write),
// lower bounds below it.
constexpr int kStatReqSegRays = kStatPacket + 3;
constexpr int kStatReqSegShadows = kStatReqSegRays + kMaxLevels;
constexpr int kStatReqRays = kStatReqSegShadows + kMaxLevels;
constexpr int kStatReqShadows = kStatReqRays + kMaxLevels;
constexpr int kNumStats = kStatReqShadows + kMaxLevels;
// counting builds: per walk launch (closest / any-hit x level) and wave {start, end (100 MHz
// ticks), rays fetched, child records fetched}, after the statistics (mrt_wave_log)
constexpr int kWaveLogWaves = 8192;
constexpr int kWaveLogEntries = 2 * kMaxLevels * kWaveLogWaves * 4;

// One level of the wavefront (SoA queues).
struct Level {
    float4* rO;      // origin xyz, w = path key bits
    float4* rD;      // direction xyz, w = source primitive code bits
    uint32_t* tree;  // vertex code in the ray tree
    float4* hit;     // t, u, v, hit primitive code bits
    int4* vtx;       // material (-1 terminal), first shadow ray, first child in the next level,
                     // shadow ray count << 3 | children (1 diffuse, 2 specular, 4 transmission,
                     // stored consecutively in that order)
    float4* res;     // resolved radiance xyz, w = "intersected light" flag
    float4* sO;      // shadow ray origin, w = source primitive bits
    float4* sD;      // shadow ray direction, w = distance to the light
    float4* sC;      // light contribution Le*cos, w = occluded flag
    // textured scenes: the texel this vertex's hit wrote into its material's Kd (xyz, w = the
    // material index, -1 none), and the last such write in the vertex's subtree (Shader.cpp:112-120)
    float4* kd;
    float4* last;
    int cap;        // physical slots: kQueueSegs * segCap (level 1: its dense paths)
    int shadowCap;  // kQueueSegs * shadowSegCap
    int segCap;     // slots per segment (Queue segments above)
    int shadowSegCap;
};

// Scenes with several textured materials: one entry per level (index = level) of the records the Kd
// replay walks (k_resolve_textures, searchLastWrite), in device memory; cap 0: no such level.
struct TexLevel {
    const int4* vtx;
    const float4* kd;
    const float4* last;
    int cap;
    int pad;
};

// Work units: rectangles of pixels (a reference tile cut into 8-row bands).  prefix[u] is
// the first pixel slot of unit u; slots inside a unit are column-major.
struct PixelMap {
    const int4* rect;    // x0, y0, width, height
    const int* prefix;   // nUnits entries
    int nUnits;
    int pad;
};

struct RaygenArgs {
    GCamera cam;
    PixelMap map;
    const float4* tables;  // .y: the sampler table
    const float2* jitter;  // per 8-entry block b: sampler[8b + kPJitterU], sampler[8b + kPJitterV]
    int width, height;
    int slotBase;    // first pixel slot of this chunk
    int nPaths;      // slots in chunk * spp
    int spp;         // samples processed in this pass
    int sppTotal;    // samplesPixel of the renderer
    int sampleBase;  // global index of the first sample of this pass
    // the pixel sampler (Renderer's samplerPixel_): 1 StaticHaltonSeq (table draws), 0 Constant
    // (every draw constJitter); C_wrapper.cpp:144-148 picks StaticHaltonSeq iff samplesPixel > 1
    int tableJitter;
    float constJitter;
    // the level-1 packet walk generating these rays (tuning key 33): 1 also stores their records,
    // 0 leaves them to k_shade to regenerate
    int storeRays;
    // A batch of views (mrt_render_views): the chunk's slots are virtual slots, view * viewSlots +
    // slot of the shard, and a path's camera is cams[view] (device memory) instead of cam.  Null for
    // a plain frame, whose kernels are instantiations of their own and never read these two.
    int viewSlots;
    const GCamera* cams;
};

struct ShadeArgs {
    int maxDepth;      // RayDepthMax
    int samplesLight;  // Config::samplesLight
    float maxPoint[3]; // DepthMap::maxPoint_ (C_wrapper.cpp:79-131 maxDist)
    unsigned long long* stats;  // counting pass only (else null): kStatShaded
};

// A level's segmented queue seen as one dense index range (k_shade, k_resolve, the per-wave walk):
// dense index v -> slot g * segCap + (v - pre[g]) of the segment holding it.  Counts are clamped to
// the segment (an overflowed pass is redone).
struct SegMap {
    int pre[kQueueSegs + 1];
    int segCap;
    __device__ __forceinline__ int total() const { return pre[kQueueSegs]; }
    __device__ __forceinline__ int phys(int v) const {
        int slot = v;  // segment 0: v - pre[0]
#pragma unroll
        for (int g = 1; g < kQueueSegs; ++g)
            if (v >= pre[g]) slot = g * segCap + (v - pre[g]);
        return slot;
    }
};
__device__ __forceinline__ SegMap segMap(const int* counters, int level, bool shadows, int segCap) {
    SegMap m;
    m.segCap = segCap;
    int acc = 0;
#pragma unroll
    for (int g = 0; g < kQueueSegs; ++g) {
        m.pre[g] = acc;
        acc += min(counters[shadows ? cntShadows(level, g) : cntRays(level, g)], segCap);
    }
    m.pre[kQueueSegs] = acc;
    return m;
}
// a dense range [0, n) as segments of segCap slots: the counts of level 1 (camera rays) and of
// rays loaded from the host (mrt_trace_rays)
__device__ __forceinline__ void denseCounts(int* counters, int level, bool shadows, int n, int segCap) {
#pragma unroll
    for (int g = 0; g < kQueueSegs; ++g)
        counters[shadows ? cntShadows(level, g) : cntRays(level, g)] = max(0, min(n - g * segCap, segCap));
}

struct AccumArgs {
    PixelMap map;
    int width;
    int slotBase;
    int nSlots;
    int spp;
    int sampleBase;
    // a batch of views (viewSlots > 0): slotBase + q is a virtual slot, view * viewSlots + slot; view
    // v's bitmap starts at v * viewPixels, the packed buffer is indexed by the virtual slot
    int viewSlots;
    int viewPixels;
};


void launchRaygen(const RaygenArgs& a, const Level& lv, int* counters, hipStream_t st);
// gen (level 1 with the packet walk, packetLevel1): the walk generates the camera rays itself and
// stores their records, replacing launchRaygen
bool packetLevel1(const DScene& s);
void launchTrace(const DScene& s, const Level& lv, int* counters, int level, int2* gstack, int gdepth,
                 unsigned long long* stats, bool countStats, int maxThreads, hipStream_t st,
                 const RaygenArgs* gen = nullptr);
void launchShadow(const DScene& s, const Level& lv, int* counters, int level, int2* gstack, int gdepth,
                  unsigned long long* stats, bool countStats, int maxThreads, hipStream_t st, int gridPct = 100);
// deadNext: level + 1 is the depth-capped last level (its rays are counted, never written)
// Level 1's ray generation, walk and shading in one launch (k_trace_packet_shade) where it applies
// (canFuseLevel1: DScene::fuseShade, the packet walk, Whitted / PathTracer, the lean shading, no
// counting); it replaces launchRaygen + launchTrace + launchShade of level 1.
bool canFuseLevel1(int shader, const DScene& s, const ShadeArgs& a);
void launchTraceShadeFused(int shader, const DScene& s, const Level& lv, const Level& nx, int* counters, int level,
                           const ShadeArgs& a, int2* gstack, int gdepth, int maxThreads, hipStream_t st, bool deadNext,
                           const RaygenArgs& ra);
// regen (level 1, Whitted / PathTracer): the camera rays are regenerated from *regen (cameraRay)
// instead of read from lv's records, which the packet walk then does not store
void launchShade(int shader, const DScene& s, const Level& lv, const Level& nx, int* counters, int level,
                 const ShadeArgs& a, int grid, hipStream_t st, bool deadNext = false,
                 const RaygenArgs* regen = nullptr);
// deadChildren: level + 1 is the depth-capped last level, whose results are all zero; its
// records are then not read (a zero child adds exactly nothing, section 3 of DESIGN.md)
// texLevels: the device table of levels (TexLevel) of a scene with several textured materials
// (DScene::textured > 1); null: the single-material replay
void launchResolve(int shader, const DScene& s, const Level& lv, const Level& nx, int* counters, int level,
                   const ShadeArgs& a, int grid, hipStream_t st, bool deadChildren = false,
                   const TexLevel* texLevels = nullptr);
void launchAccumulate(const AccumArgs& a, const float4* res, int32_t* bitmap, int32_t* packed, hipStream_t st);
// level 1's resolve and the accumulation in one launch (Whitted / PathTracer; false: not launched)
bool launchResolveAccumulate(int shader, const DScene& s, const Level& lv, const Level& nx, const ShadeArgs& sa,
                             bool deadChildren, const AccumArgs& a, int32_t* bitmap, int32_t* packed, hipStream_t st,
                             const TexLevel* texLevels = nullptr);
// rank 0's frame assembly: up to kUnpackRanks shards per launch (rank first + k reads row first + k
// of the gathered array, stride entries apart)
constexpr int kUnpackRanks = 16;
struct UnpackArgs {
    PixelMap maps[kUnpackRanks];
    int n[kUnpackRanks];
    int width;
    int first;
    int stride;
    int pad;
};
void launchUnpackRanks(const UnpackArgs& a, int ranks, int maxN, const int32_t* gathered, int32_t* bitmap,
                       hipStream_t st);
void launchDumpHits(const Level& lv, int n, int32_t* kind, int32_t* index, float* t, hipStream_t st);
// hostOut (pinned host memory, kNumStats entries): the statistics copied there and the counters reset
// (and with zeroStats the statistics too), for the next chunk or pass
void launchTally(int* counters, int maxLevel, unsigned long long* stats, hipStream_t st, int skippedLevel = 0,
                 unsigned long long* hostOut = nullptr, bool zeroStats = false);
// known-answer kernels (device slab / triangle tests) and arbitrary-ray loading for tests
void launchKatSlab(const float* boxes, const float* orig, const float* dir, int n, int32_t* out, hipStream_t st);
void launchKatTriangle(const float* tris, const float* orig, const float* dir, int n, int32_t* hit, float* t,
                       hipStream_t st);
void launchLoadRays(const Level& lv, const float* orig, const float* dir, const float* dist, const uint32_t* src, int n,
                    bool any, int* counters, hipStream_t st);
// Ray queries (mrt_cast_rays_device).  A chunk of the caller's device-resident batch: ray base + i
// (i < n, the launch's count) is read at orig + (base + i) * origStride, its source pair at
// src + 2 (base + i); 64-bit, the batch may hold 2^31 - 1 rays of any stride.
struct QueryRays {
    const float* orig;
    const float* dir;
    const float* dist;   // any hit: tmax per ray; else not read
    const int32_t* src;  // (kind, input index) pairs, or null
    long long origStride, dirStride;  // in floats
    long long base;
};
// The scene's primitive orders on the device: *Inv[input index] = BVH-order index (a source pair ->
// the walk's primitive code), *Order[BVH-order index] = input index (a hit -> the caller's index),
// and each kind's count (a source pair outside it names nothing).  Lights keep their input order.
struct QueryTables {
    const int32_t* triInv;
    const int32_t* planeInv;
    const int32_t* sphereInv;
    const int32_t* triOrder;
    const int32_t* planeOrder;
    const int32_t* sphereOrder;
    int32_t nTri, nPlanes, nSpheres, nLights;
};
// k_query_load: n rays of q into lv's queue (rO / rD / tree, or with any sO / sD / sC) with the dense
// segment counts, as launchLoadRays; n at most lv.cap (any: lv.shadowCap)
void launchQueryLoad(const Level& lv, const QueryRays& q, const QueryTables& tb, int n, bool any, int* counters,
                     hipStream_t st);
// k_query_store: the walk's results of those n rays to kind / index / t at base + i (null: not
// written); any: kind = occluded, nothing else
void launchQueryStore(const Level& lv, const QueryTables& tb, int n, bool any, long long base, int32_t* kind,
                      int32_t* index, float* t, hipStream_t st);
// Surface records (mrt_cast_hits_device): the device arrays of mrt_hit_records, each packed (ray g's
// record at g * width) or null (not wanted: neither gathered nor stored).
struct HitRecords {
    int32_t* kind;
    int32_t* index;
    float* t;
    float* bary;      // 2
    float* point;     // 3
    float* normal;    // 3
    float* texCoord;  // 2
    int32_t* material;
    float* kd;        // 3
    float* ks;        // 3
    float* kt;        // 3
    float* le;        // 3
    float* ior;
    bool beyondHit() const { return beyondGeometry() || bary != nullptr || point != nullptr; }  // more than k_query_store writes
    bool beyondGeometry() const {
        return normal != nullptr || texCoord != nullptr || material != nullptr || kd != nullptr || ks != nullptr ||
               kt != nullptr || le != nullptr || ior != nullptr;
    }
};
// k_query_store_hits: the closest-hit walk's results of those n rays as surface records at base + i: what
// k_query_store writes, then the hit's geometry and material through the shading's own device functions
// (hitGeometry, hitMaterial, textureWrite).  Two instantiations: geometry only (kind, index, t, bary,
// point: no shading or material record is fetched) where out.beyondGeometry() is false, else the full one.
void launchQueryStoreHits(const DScene& s, const Level& lv, const QueryTables& tb, int n, long long base,
                          const HitRecords& out, hipStream_t st);
// Multi-hit queries (mrt_cast_multi_hits_device): the device arrays of mrt_multi_hits, packed (ray g's
// count at g, its entry k at g * K + k, two floats per entry of bary) or null (not wanted: not stored).
constexpr int kMultiHitsMax = 16;  // MRT_MULTI_HITS_MAX: the largest K-buffer
struct MultiHits {
    int32_t* count;
    int32_t* kind;
    int32_t* index;
    float* t;
    float* bary;
};
// k_multi_walk (mrt_multi_hit.hpp): the n rays k_query_load put into lv's queue walked with no cull,
// each ray's first K hits (K 1 .. 16) in order, its hit count and the padding stored by the walk itself
// at base + i, indices mapped to input order through tb.  dist: the caller's tmax array (ray base + i's
// at dist[base + i]) or null (RayLengthMax).  The spill area is the closest-hit walk's (gstack, gdepth
// entries for each of maxThreads threads): the grid holds at most maxThreads threads.
void launchMultiWalk(const DScene& s, const Level& lv, int* counters, int2* gstack, int gdepth, const QueryTables& tb,
                     const float* dist, long long base, int n, int K, const MultiHits& out, int maxThreads,
                     hipStream_t st);
// Nearest-point queries (mrt_nearest_points_device): the device arrays of mrt_nearest, packed (point g's
// kind at g, its nearest point at 3 g, its bary at 2 g) or null (not wanted: not stored).
struct Nearest {
    int32_t* kind;
    int32_t* index;
    float* dist2;
    float* point;  // 3
    float* bary;   // 2
    int32_t* tests;
};
// k_nearest_walk (mrt_nearest.hpp): the n points k_query_load put into lv's queue (the origins; the
// direction slots are not read, rD.w is the mapped source) answered by the walk and stored by it at
// base + i, indices mapped to input order through tb.  dist: the caller's radius array (point base + i's
// at dist[base + i]) or null (unbounded).  The spill area is the closest-hit walk's, as launchMultiWalk's.
void launchNearestWalk(const DScene& s, const Level& lv, int* counters, int2* gstack, int gdepth, const QueryTables& tb,
                       const float* dist, long long base, int n, const Nearest& out, int maxThreads, hipStream_t st);
// Neighbour queries (mrt_neighbours_device): the device arrays of mrt_neighbours, packed (point g's count
// and tests at g, its entry k at g * K + k, three floats per entry of point, two of bary) or null (not
// wanted: not stored).
constexpr int kNeighboursMax = 16;  // MRT_NEIGHBOURS_MAX: the largest list
struct Neighbours {
    int32_t* count;
    int32_t* kind;
    int32_t* index;
    float* dist2;
    float* point;  // 3
    float* bary;   // 2
    int32_t* tests;
};
// k_neighbour_walk (mrt_neighbours.hpp): the n points k_query_load put into lv's queue, as
// launchNearestWalk's, each point's first K accepted candidates (K 1 .. 16) in order, its count and the
// padding stored by the walk itself at base + i.  Where out.count is null the walk is the K-nearest search
// (its bound shrinks to the list's K-th entry); where it is wanted the bound stays the point's radius.
void launchNeighbourWalk(const DScene& s, const Level& lv, int* counters, int2* gstack, int gdepth, const QueryTables& tb,
                         const float* dist, long long base, int n, int K, const Neighbours& out, int maxThreads,
                         hipStream_t st);
// Overlap queries (mrt_overlap_boxes_device): the device arrays of mrt_overlaps, packed (box g's any, count
// and tests at g, its entry k at g * K + k) or null (not wanted: not stored).
constexpr int kOverlapMax = 16;  // MRT_OVERLAP_MAX: the largest list
struct Overlaps {
    int32_t* any;
    int32_t* count;
    int32_t* kind;
    int32_t* index;
    int32_t* tests;
};
// k_overlap_walk (mrt_overlap.hpp): the n boxes k_query_load put into lv's queue (mn the origins, mx the
// directions), each box's first K accepted candidates (K 1 .. 16) in (kind, input index) order, its count
// and the padding stored by the walk itself at base + i.  Where count, kind and index are all null the walk
// stops at a lane's first acceptance (the occupancy test); the spill area is the closest-hit walk's.
void launchOverlapWalk(const DScene& s, const Level& lv, int* counters, int2* gstack, int gdepth, const QueryTables& tb,
                       long long base, int n, int K, const Overlaps& out, int maxThreads, hipStream_t st);
// known answers: pair i (kind's record at prims + i * pointPrimFloats(kind), box at boxes + 6 i) through the
// device's overlap functions
void launchKatBoxOverlap(int kind, const float* prims, const float* boxes, int n, int32_t* out, hipStream_t st);
// k_triangle_overlap_walk (mrt_triangle_overlap.hpp): the n query triangles whose corners a and b k_query_load
// put into lv's queue (a the origins, b the directions) and whose corner c the walk reads from the caller's
// array (triangle base + i's at c + (base + i) * cStride), answered and stored as launchOverlapWalk's boxes.
void launchTriangleOverlapWalk(const DScene& s, const Level& lv, int* counters, int2* gstack, int gdepth,
                               const QueryTables& tb, const float* c, long long cStride, long long base, int n, int K,
                               const Overlaps& out, int maxThreads, hipStream_t st);
// known answers: pair i (kind's record at prims + i * pointPrimFloats(kind), triangle at tris + 9 i) through the
// device's triangle overlap functions
void launchKatTriangleOverlap(int kind, const float* prims, const float* tris, int n, int32_t* out, hipStream_t st);
// Sweep queries (mrt_sweep_spheres_device): the device arrays of mrt_sweeps, packed (ray g's hit, kind, index,
// t and tests at g, its centre and contact point at 3 g, its bary at 2 g) or null (not wanted: not stored).
struct Sweeps {
    int32_t* hit;
    int32_t* kind;
    int32_t* index;
    float* t;
    float* centre;  // 3
    float* point;   // 3
    float* bary;    // 2
    int32_t* tests;
};
// k_sweep_walk (mrt_sweep.hpp): the n rays k_query_load put into lv's queue (rD.w the mapped source) swept
// with the radius at radius[base + i] up to dist[base + i] (dist null: unbounded) and stored by the walk at
// base + i, indices mapped to input order through tb.  Where only hit is wanted (tests aside) the walk stops
// at a lane's first acceptance; the spill area is the closest-hit walk's.
void launchSweepWalk(const DScene& s, const Level& lv, int* counters, int2* gstack, int gdepth, const QueryTables& tb,
                     const float* radius, const float* dist, long long base, int n, const Sweeps& out, int maxThreads,
                     hipStream_t st);
// known answers: pair i (kind's record at prims + i * pointPrimFloats(kind), sweep o, d, r at rays + 7 i)
// through the device's sweep functions
void launchKatSphereSweep(int kind, const float* prims, const float* rays, int n, int32_t* hit, float* t, float* centre,
                          float* point, float* bary, hipStream_t st);
// known answers: pair i (kind's record at prims + i * pointPrimFloats(kind), point at points + 3 i)
// through the device's distance functions
void launchKatPointDistance(int kind, const float* prims, const float* points, int n, float* dist2, float* nearest,
                            float* bary, hipStream_t st);
// Shaded ray queries (mrt_shade_rays_device).  k_query_load's keyed form: n rays of q into lv's queue
// as level-1 records of a frame's kind - rO.w the path key (keys[base + i]; null: pathKey(base + i, 0)),
// rD.w the mapped source, tree = 1 - with the dense segment counts.
void launchShadeLoad(const Level& lv, const QueryRays& q, const QueryTables& tb, int n, const uint32_t* keys,
                     int* counters, hipStream_t st);
// k_resolve_store: level 1's resolve and the store of its n paths' radiance in one launch, path i to
// rgb + (base + i) * stride (floats) - launchResolveAccumulate's value without the fold into pixels
// (Whitted / PathTracer; false: not launched)
bool launchResolveStore(int shader, const DScene& s, const Level& lv, const Level& nx, const ShadeArgs& sa,
                        bool deadChildren, int n, long long base, float* rgb, long long stride, hipStream_t st,
                        const TexLevel* texLevels = nullptr);
// k_radiance_store: the same store from level 1's radiance records
void launchRadianceStore(const float4* res, int n, long long base, float* rgb, long long stride, hipStream_t st);
// k_camera_rays: path p's camera ray (cameraRay with a.cam, as k_raygen's record) packed xyz to
// orig / dir + 3 p, its path key and pixel y * width + x; null outputs are not written
void launchCameraRays(const RaygenArgs& a, float* orig, float* dir, uint32_t* key, int32_t* pixel, hipStream_t st);
int traceResidentThreadsPerCU();  // max over the trace walks of resident threads per CU
// out[2 slot], out[2 slot + 1] = real-time counter (100 MHz) before / after a spin of `ticks`
void launchSpin(unsigned long long* out, int slot, unsigned long long ticks, hipStream_t st);

}  // namespace mrt
