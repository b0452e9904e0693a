// ORACLE — TEST INFRASTRUCTURE ONLY.  Only tests/, __graft_entry__.smoke() and bench.py's
// cpu_baseline leg may load this library; the product path (libmobilert_amd.so) never does.
//
// A CPU restatement of the MobileRT render path (TiagoMSSantos/MobileRayTracer, snapshot
// 2025-01-17), written from the reference's behaviour, structured like the reference:
// AoS primitives, by-value Intersection records threaded through every primitive test,
// recursive Whitted / PathTracer shading, a std::thread tile loop with an atomic tile
// counter.  It is the parity oracle for the HIP kernels and, run multi-threaded, the
// "port" CPU baseline of bench.py.
//
// Why a restatement: the reference cannot be compiled here (its glm / tinyobjloader / boost
// submodules are empty and its CMake build fetches them from the network).
// Pinned against the reference's own tests: the numeric assertions of
// app/Unit_Testing/TestTriangle.cpp, TestAABB.cpp, TestPlane.cpp, TestRay.cpp and
// TestCameraLoader.cpp, the triangle/light-count KAT of scripts/test/docker/dockerfile.sh
// (CornellBox-Water 7088 faces / 2 lights), and glibc's std::partition (the BVH build uses a
// restated libstdc++ partition, checked against std::partition by oracle_selftest_partition).
// glm 1.0.1 and tinyobjloader v1.0.7 arithmetic is restated.  The reference
// holds no golden image, but its core does compile against the stand-in headers of oracle/refshim/
// (oracle/ref_build.py): frames, ray batches, builds, camera rays, primitive tests and the pixel
// conversion recorded from it are fixtures in tests/golden/reference/ that this file must reproduce
// bit for bit (tests/test_reference_fixtures_cpu.py).  Unpinned beyond that: what draws from the
// sample tables (area lights, PathTracer, spp > 1), the loader and textures.
//
// Deliberate deviations from the reference, identical in the product:
//   * sample tables use fixed seeds and every draw is a pure function of
//     (pixel, sample, ray-tree vertex, purpose) instead of shared atomic cursors;
//   * the OBJ fill is single-threaded in file order; a textured hit writes Kd into the render
//     thread's own copy of the materials (the reference shares them between threads);
//   * each pixel receives its samples in order (no tile-claim race, Renderer.cpp:190-193).
#include <algorithm>
#include <limits>
#include <map>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace oracle {

// ---- constants (app/MobileRT/Utils/Constants.hpp) ----------------------------------------
const float Epsilon = 1.0e-06F;
const float EpsilonLarge = 1.0e-05F;
const float RayLengthMax = 1.0e+30F;
const int RayDepthMin = 1;
const int NumberOfTiles = 256;
const uint32_t ArrayMask = 0xFFFFF;
const uint32_t ArraySize = ArrayMask + 1;
const float kTwoPi = 6.28318530717958647692528676655900576f;
const float kQuarterPi = 0.785398163397448309615660845819875721f;
const float kPi = 3.14159265358979323846264338327950288f;

// ---- glm-like vectors ------------------------------------------------------------------
struct Vec3 {
    float v[3];
    Vec3() : v{0, 0, 0} {}
    Vec3(float a, float b, float c) : v{a, b, c} {}
    explicit Vec3(float s) : v{s, s, s} {}
    float& operator[](int i) { return v[i]; }
    float operator[](int i) const { return v[i]; }
};
inline Vec3 operator+(const Vec3& a, const Vec3& b) { return Vec3(a[0] + b[0], a[1] + b[1], a[2] + b[2]); }
inline Vec3 operator-(const Vec3& a, const Vec3& b) { return Vec3(a[0] - b[0], a[1] - b[1], a[2] - b[2]); }
inline Vec3 operator*(const Vec3& a, const Vec3& b) { return Vec3(a[0] * b[0], a[1] * b[1], a[2] * b[2]); }
inline Vec3 operator*(const Vec3& a, float s) { return Vec3(a[0] * s, a[1] * s, a[2] * s); }
inline Vec3 operator*(float s, const Vec3& a) { return Vec3(s * a[0], s * a[1], s * a[2]); }
inline Vec3 operator/(const Vec3& a, float s) { return Vec3(a[0] / s, a[1] / s, a[2] / s); }
inline Vec3& operator+=(Vec3& a, const Vec3& b) { a = a + b; return a; }
inline Vec3& operator*=(Vec3& a, const Vec3& b) { a = a * b; return a; }
inline Vec3& operator/=(Vec3& a, float s) { a = a / s; return a; }
inline float dot(const Vec3& a, const Vec3& b) {
    const Vec3 t = a * b;  // glm compute_dot: tmp = a * b; tmp.x + tmp.y + tmp.z
    return t[0] + t[1] + t[2];
}
inline Vec3 cross(const Vec3& x, const Vec3& y) {
    return Vec3(x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]);
}
inline float length(const Vec3& v) { return std::sqrt(dot(v, v)); }
inline Vec3 normalize(const Vec3& v) { return v * (1.0F / std::sqrt(dot(v, v))); }
inline Vec3 reflect(const Vec3& i, const Vec3& n) { return i - n * dot(n, i) * 2.0F; }
inline Vec3 refract(const Vec3& i, const Vec3& n, float eta) {
    const float d = dot(n, i);
    const float k = 1.0F - eta * eta * (1.0F - d * d);
    return (k >= 0.0F) ? (eta * i - (eta * d + std::sqrt(k)) * n) : Vec3(0.0F);
}
inline Vec3 vmin(const Vec3& a, const Vec3& b) {  // glm::min(x, y) = y < x ? y : x
    return Vec3(std::min(a[0], b[0]), std::min(a[1], b[1]), std::min(a[2], b[2]));
}
inline Vec3 vmax(const Vec3& a, const Vec3& b) {
    return Vec3(std::max(a[0], b[0]), std::max(a[1], b[1]), std::max(a[2], b[2]));
}
inline bool hasPositiveValue(const Vec3& v) { return v[0] > 0 || v[1] > 0 || v[2] > 0; }
struct Vec2 {
    float x, y;
};
inline Vec2 operator*(const Vec2& a, float s) { return Vec2{a.x * s, a.y * s}; }
inline Vec2 operator+(const Vec2& a, const Vec2& b) { return Vec2{a.x + b.x, a.y + b.y}; }

// Texture (Texture.cpp): 8-bit channels as stb_image returns them.  The oracle does not decode
// images itself: oracle.py decodes PNGs (its own decoder) and registers them by path.
struct Texture {
    int32_t width = 0, height = 0, channels = 0;
    std::vector<uint8_t> image;
    Vec3 loadColor(const Vec2& tc) const {  // Texture.cpp:37-48
        const int32_t u = static_cast<int32_t>(tc.x * width);
        const int32_t v = static_cast<int32_t>(tc.y * height);
        size_t index = static_cast<uint32_t>(v * width * channels + u * channels);
        if (index + 3 > image.size()) index = image.size() >= 3 ? image.size() - 3 : 0;  // the reference reads past the end
        return Vec3(static_cast<float>(image[index + 0]) / 255.0F, static_cast<float>(image[index + 1]) / 255.0F,
                    static_cast<float>(image[index + 2]) / 255.0F);
    }
};
std::map<std::string, Texture>& textureRegistry() {
    static std::map<std::string, Texture> r;
    return r;
}

bool equalF(float a, float b) { return std::fabs(a - b) < Epsilon; }
bool equalV(const Vec3& a, const Vec3& b) { return equalF(a[0], b[0]) && equalF(a[1], b[1]) && equalF(a[2], b[2]); }

// ---- deterministic sample streams (shared definition with the product) -------
uint32_t hash32(uint32_t x) {
    x ^= x >> 16u;
    x *= 0x7feb352du;
    x ^= x >> 15u;
    x *= 0x846ca68bu;
    x ^= x >> 16u;
    return x;
}
uint32_t pathKey(uint32_t pixelIndex, uint32_t globalSample) {
    return hash32(pixelIndex * 0x9E3779B9u ^ hash32(globalSample + 0x632BE5ABu));
}
uint32_t sampleIndex(uint32_t key, uint32_t treeCode, uint32_t purpose) {
    // a vertex's draws: consecutive entries from a hashed start aligned to 8 entries
    return ((hash32(key ^ hash32(treeCode * 0x9E3779B9u + 0x7F4A7C15u)) & ~7u) + purpose) & ArrayMask;
}
enum Purpose : uint32_t { P_JITTER_U = 0, P_JITTER_V = 1, P_RUSSIAN = 0, P_HEMI1 = 1, P_HEMI2 = 2, P_LIGHT = 3 };

float haltonSequence(uint32_t index, uint32_t base) {  // Utils.cpp:43-53
    float fraction = 1.0F;
    float nextValue = 0.0F;
    const float baseInFloat = static_cast<float>(base);
    while (index > 0) {
        fraction /= baseInFloat;
        nextValue += fraction * static_cast<float>(index % base);
        index = static_cast<uint32_t>(std::floor(index / base));
    }
    return nextValue;
}

// Shader.cpp:206-212: cos / sin of phi = two_pi * r1 through libm (std::cos / std::sin of a
// float = cosf / sinf); out of line, so both calls stay plain libm calls
__attribute__((noinline)) void hemisphereTrig(float r1, float* c, float* s) {
    const float phi = kTwoPi * r1;
    *c = std::cos(phi);
    *s = std::sin(phi);
}

std::vector<float> haltonTable(uint32_t seed) {  // Utils.hpp:209-218, fixed seed
    std::vector<float> t(ArraySize);
    for (uint32_t i = 0; i < ArraySize; ++i) t[i] = haltonSequence(i, 2);
    std::mt19937 generator(seed);
    std::shuffle(t.begin(), t.end(), generator);
    return t;
}

int32_t incrementalAvg(const Vec3& sample, int32_t avg, int32_t numSample) {  // Utils.cpp:66-90
    const uint32_t avgUnsigned = static_cast<uint32_t>(avg);
    const uint32_t numSampleUnsigned = static_cast<uint32_t>(numSample);
    const uint32_t lastRed = avgUnsigned & 0xFFU;
    const uint32_t lastGreen = (avgUnsigned >> 8U) & 0xFFU;
    const uint32_t lastBlue = (avgUnsigned >> 16U) & 0xFFU;
    const uint32_t samplerRed = static_cast<uint32_t>(sample[0] * 255U);
    const uint32_t samplerGreen = static_cast<uint32_t>(sample[1] * 255U);
    const uint32_t samplerBlue = static_cast<uint32_t>(sample[2] * 255U);
    const uint32_t currentRed = ((numSampleUnsigned - 1U) * lastRed + samplerRed) / numSampleUnsigned;
    const uint32_t currentGreen = ((numSampleUnsigned - 1U) * lastGreen + samplerGreen) / numSampleUnsigned;
    const uint32_t currentBlue = ((numSampleUnsigned - 1U) * lastBlue + samplerBlue) / numSampleUnsigned;
    const uint32_t retR = std::min(currentRed, 255U);
    const uint32_t retG = std::min(currentGreen, 255U);
    const uint32_t retB = std::min(currentBlue, 255U);
    return static_cast<int32_t>(0xFF000000 | retB << 16U | retG << 8U | retR);
}

// ---- Ray / Intersection ------------------------------------------------------------------
struct RenderCtx;

struct Ray {  // Ray.hpp:19-45
    Vec3 origin, direction;
    int32_t depth;
    const void* primitive;
    bool shadowTrace;
    Ray(const Vec3& dir, const Vec3& org, int32_t d, bool shadow, const void* prim, std::atomic<uint64_t>* counter)
        : origin(org), direction(dir), depth(d), primitive(prim), shadowTrace(shadow) {
        if (counter != nullptr) counter->fetch_add(1, std::memory_order_relaxed);  // Ray.cpp:25-28, :57
    }
};

struct Material {  // Material.hpp:18-43
    Vec3 Le, Kd, Ks, Kt;
    float ior = 1.0F;
    std::string texture;          // map_Kd name ("" none)
    const Texture* tex = nullptr;
    Material() = default;
    Material(Vec3 kd, Vec3 ks = Vec3(), Vec3 kt = Vec3(), float r = 1.0F, Vec3 le = Vec3()) : Le(le), Kd(kd), Ks(ks), Kt(kt), ior(r) {}
    bool operator==(const Material& o) const {  // Material.cpp:36-45
        return equalV(Kd, o.Kd) && equalV(Ks, o.Ks) && equalV(Kt, o.Kt) && equalV(Le, o.Le) && equalF(ior, o.ior) &&
               texture == o.texture;
    }
};

struct Intersection {  // Intersection.hpp:16-27, copied by value through every test
    Vec3 point;
    Vec3 normal{0.0F, 1.0F, 0.0F};
    const Material* material = nullptr;
    float length = RayLengthMax;
    const void* primitive = nullptr;
    int32_t materialIndex = -1;
    int kind = 0;      // oracle bookkeeping for hit-id dumps: 1 plane 2 sphere 3 triangle 4 light
    int64_t index = -1;
    Vec2 texCoords{-1.0F, -1.0F};
    Ray ray;
    Intersection(Ray r, float dist = RayLengthMax) : length(dist), ray(r) {}
};

// ---- AABB (AABB.cpp) --------------------------------------------------------------------
struct AABB {
    Vec3 pointMin, pointMax;
    bool intersect(const Ray& ray) const {  // AABB.cpp:34-54
        const float invDirX = 1.0F / ray.direction[0];
        const float rayOrgX = ray.origin[0];
        const float t1X = (pointMin[0] - rayOrgX) * invDirX;
        const float t2X = (pointMax[0] - rayOrgX) * invDirX;
        float tMin = std::min(t1X, t2X);
        float tMax = std::max(t1X, t2X);
        for (int axis = 1; axis < 3; ++axis) {
            const float invDir = 1.0F / ray.direction[axis];
            const float rayOrg = ray.origin[axis];
            const float t1 = (pointMin[axis] - rayOrg) * invDir;
            const float t2 = (pointMax[axis] - rayOrg) * invDir;
            tMin = std::max(tMin, std::min(t1, t2));
            tMax = std::min(tMax, std::max(t1, t2));
        }
        return tMax >= std::max(tMin, 0.0F);
    }
    float surfaceArea() const {  // AABB.cpp:61-71
        const Vec3 l = pointMax - pointMin;
        const float bottomTopArea = 2 * l[0] * l[2];
        const float sideAreaXY = 2 * l[0] * l[1];
        const float sideAreaZY = 2 * l[2] * l[1];
        return bottomTopArea + sideAreaXY + sideAreaZY;
    }
    Vec3 centroid() const { return pointMin + (pointMax - pointMin) / 2.0F; }
};
AABB surroundingBox(const AABB& a, const AABB& b) { return AABB{vmin(a.pointMin, b.pointMin), vmax(a.pointMax, b.pointMax)}; }

// ---- shapes ------------------------------------------------------------------------------
struct Triangle {  // Triangle.hpp:18-27 (AoS, 100 bytes of payload)
    Vec3 AC, AB, pointA, normalA, normalB, normalC;
    Vec2 texA{-1, -1}, texB{-1, -1}, texC{-1, -1};
    int32_t materialIndex = -1;
    int64_t inputIndex = -1;

    static Triangle build(const Vec3& a, const Vec3& b, const Vec3& c, const Vec3* na, const Vec3* nb, const Vec3* nc,
                          int32_t mat) {
        Triangle t;  // Builder (Triangle.cpp:328-339) then ctor (Triangle.cpp:14-26)
        t.AC = c - a;
        t.AB = b - a;
        t.pointA = a;
        const Vec3 flat = normalize(cross(t.AC, t.AB));
        t.normalA = normalize(na ? *na : flat);
        t.normalB = normalize(nb ? *nb : flat);
        t.normalC = normalize(nc ? *nc : flat);
        t.materialIndex = mat;
        return t;
    }
    Intersection intersect(Intersection intersection) const {  // Triangle.cpp:63-109
        if (intersection.ray.primitive == this) return intersection;
        const Vec3 perpendicularVector = cross(intersection.ray.direction, AC);
        const float normalizedProjection = dot(AB, perpendicularVector);
        if (std::abs(normalizedProjection) < Epsilon) return intersection;
        const float normalizedProjectionInv = 1.0F / normalizedProjection;
        const Vec3 vectorToCamera = intersection.ray.origin - pointA;
        const float u = normalizedProjectionInv * dot(vectorToCamera, perpendicularVector);
        if (u < 0.0F || u > 1.0F) return intersection;
        const Vec3 upPerpendicularVector = cross(vectorToCamera, AB);
        const float v = normalizedProjectionInv * dot(intersection.ray.direction, upPerpendicularVector);
        if (v < 0.0F || (u + v) > 1.0F) return intersection;
        const float distanceToIntersection = normalizedProjectionInv * dot(AC, upPerpendicularVector);
        if (distanceToIntersection < Epsilon || distanceToIntersection >= intersection.length) return intersection;
        const float w = 1.0F - u - v;
        Intersection res(intersection.ray, distanceToIntersection);
        res.normal = normalize(normalA * w + normalB * u + normalC * v);
        res.texCoords = texA * w + texB * u + texC * v;
        res.point = intersection.ray.origin + intersection.ray.direction * distanceToIntersection;
        res.primitive = this;
        res.materialIndex = materialIndex;
        res.kind = 3;
        res.index = inputIndex;
        return res;
    }
    AABB getAABB() const {  // Triangle.cpp:116-123
        const Vec3 pointB = pointA + AB;
        const Vec3 pointC = pointA + AC;
        return AABB{vmin(pointA, vmin(pointB, pointC)), vmax(pointA, vmax(pointB, pointC))};
    }
};

struct Plane {  // Plane.cpp
    Vec3 normal, point;
    int32_t materialIndex;
    int64_t inputIndex = -1;
    Plane(const Vec3& p, const Vec3& n, int32_t m) : normal(normalize(n)), point(p), materialIndex(m) {}
    Intersection intersect(Intersection intersection) const {  // Plane.cpp:38-72
        if (intersection.ray.primitive == this) return intersection;
        const float normalizedProjection = dot(normal, intersection.ray.direction);
        if (std::abs(normalizedProjection) < Epsilon) return intersection;
        const Vec3 vecToPlane = point - intersection.ray.origin;
        const float scalarProjection = dot(normal, vecToPlane);
        const float distanceToIntersection = scalarProjection / normalizedProjection;
        if (distanceToIntersection < Epsilon || distanceToIntersection >= intersection.length) return intersection;
        Intersection res(intersection.ray, distanceToIntersection);
        res.point = intersection.ray.origin + intersection.ray.direction * distanceToIntersection;
        res.normal = normal;
        res.primitive = this;
        res.materialIndex = materialIndex;
        res.kind = 1;
        res.index = inputIndex;
        return res;
    }
    Vec3 rightVector() const {  // Plane.cpp:79-96
        Vec3 right;
        if (normal[0] >= 1) right = Vec3(0, 1, 1);
        else if (normal[1] >= 1) right = Vec3(1, 0, 1);
        else if (normal[2] >= 1) right = Vec3(1, 1, 0);
        else if (normal[0] <= -1) right = Vec3(0, 1, 1);
        else if (normal[1] <= -1) right = Vec3(1, 0, 1);
        else if (normal[2] <= -1) right = Vec3(1, 1, 0);
        return normalize(right);
    }
    AABB getAABB() const {  // Plane.cpp:103-109
        const Vec3 rightDir = rightVector();
        return AABB{point + rightDir * -100.0F, point + rightDir * 100.0F};
    }
};

struct Sphere {  // Sphere.cpp
    Vec3 center;
    float sqRadius;
    int32_t materialIndex;
    int64_t inputIndex = -1;
    Sphere(const Vec3& c, float r, int32_t m) : center(c), sqRadius(r * r), materialIndex(m) {}
    Intersection intersect(Intersection intersection) const {  // Sphere.cpp:42-81
        const Vec3 originToCenter = center - intersection.ray.origin;
        const float projectionOnDirection = dot(originToCenter, intersection.ray.direction);
        const float originToCenterMagnitude = length(originToCenter);
        const float a = dot(intersection.ray.direction, intersection.ray.direction);
        const float b = 2.0F * -projectionOnDirection;
        const float c = originToCenterMagnitude * originToCenterMagnitude - sqRadius;
        const float discriminant = b * b - 4.0F * a * c;
        if (discriminant < 0.0F) return intersection;
        const float rootDiscriminant = std::sqrt(discriminant);
        const float d1 = -b + rootDiscriminant;
        const float d2 = -b - rootDiscriminant;
        const float distanceToIntersection = std::min(d1, d2) / (2.0F * a);
        if (distanceToIntersection < EpsilonLarge || distanceToIntersection >= intersection.length) return intersection;
        Intersection res(intersection.ray, distanceToIntersection);
        res.point = intersection.ray.origin + intersection.ray.direction * distanceToIntersection;
        res.normal = normalize(res.point - center);
        res.primitive = nullptr;
        res.materialIndex = materialIndex;
        res.kind = 2;
        res.index = inputIndex;
        return res;
    }
    AABB getAABB() const {  // Sphere.cpp:88-94
        const float radius = std::sqrt(sqRadius);
        return AABB{center - Vec3(radius), center + Vec3(radius)};
    }
};

// ---- BVH (BVH.hpp) -----------------------------------------------------------------------
// libstdc++'s std::partition, bidirectional overload (bits/stl_algo.h), restated.
template <typename It, typename Pred>
It libstdcxxPartition(It first, It last, Pred pred) {
    while (true) {
        while (true) {
            if (first == last) return first;
            else if (pred(*first)) ++first;
            else break;
        }
        --last;
        while (true) {
            if (first == last) return first;
            else if (!bool(pred(*last))) --last;
            else break;
        }
        std::iter_swap(first, last);
        ++first;
    }
}

template <typename T>
struct BVH {
    struct BuildNode {
        AABB box;
        Vec3 centroid;
        int32_t oldIndex;
    };
    struct Node {
        AABB box;
        int32_t indexOffset = 0;
        int32_t numPrimitives = 0;
    };
    std::vector<Node> boxes;
    std::vector<T> primitives;

    static int32_t splitIndexSah(const std::vector<AABB>& b) {  // BVH.hpp:398-439
        const long numberBoxes = static_cast<long>(b.size());
        const long numBoxes = numberBoxes - 1;
        std::vector<float> leftArea(static_cast<size_t>(numBoxes)), rightArea(static_cast<size_t>(numBoxes));
        AABB leftBox = b[0];
        leftArea[0] = leftBox.surfaceArea();
        for (int32_t i = 1; i < numBoxes; ++i) {
            leftBox = surroundingBox(leftBox, b[static_cast<size_t>(i)]);
            leftArea[static_cast<size_t>(i)] = leftBox.surfaceArea();
        }
        AABB rightBox = b[static_cast<size_t>(numBoxes)];
        rightArea[static_cast<size_t>(numBoxes - 1)] = rightBox.surfaceArea();
        for (long i = numBoxes - 2; i >= 0; --i) {
            rightBox = surroundingBox(rightBox, b[static_cast<size_t>(i + 1)]);
            rightArea[static_cast<size_t>(i)] = rightBox.surfaceArea();
        }
        int32_t splitIndex = 1;
        float minSah = leftArea[0] + numBoxes * rightArea[0];
        for (int32_t i = 1; i < numBoxes; ++i) {
            const int32_t nextSplit = i + 1;
            const long numBoxesLeft = nextSplit;
            const long numBoxesRight = numberBoxes - numBoxesLeft;
            const float sah = numBoxesLeft * leftArea[static_cast<size_t>(i)] + numBoxesRight * rightArea[static_cast<size_t>(i)];
            if (sah < minSah) {
                splitIndex = nextSplit;
                minSah = sah;
            }
        }
        return splitIndex;
    }

    explicit BVH(std::vector<T> prims) {  // BVH.hpp:126-283
        if (prims.empty()) {
            boxes.emplace_back(Node{});
            return;
        }
        const size_t n = prims.size();
        boxes.resize(n * 2 - 1);
        std::vector<BuildNode> bn;
        bn.reserve(n);
        for (size_t i = 0; i < n; ++i) {
            const AABB box = prims[i].getAABB();
            bn.push_back(BuildNode{box, box.centroid(), static_cast<int32_t>(i)});
        }
        std::vector<int32_t> stIdx(1, 0), stBegin(1, 0), stEnd(1, 0);
        int32_t current = 0, begin = 0, end = static_cast<int32_t>(n), maxNodeIndex = 0;
        do {
            AABB sur{bn[static_cast<size_t>(begin)].box.pointMin, bn[static_cast<size_t>(begin)].box.pointMax};
            for (int32_t i = begin + 1; i < end; ++i) sur = surroundingBox(sur, bn[static_cast<size_t>(i)].box);
            const Vec3 maxDist = sur.pointMax - sur.pointMin;
            const int longestAxis = maxDist[0] >= maxDist[1] && maxDist[0] >= maxDist[2]
                                        ? 0
                                        : maxDist[1] >= maxDist[0] && maxDist[1] >= maxDist[2] ? 1 : 2;
            const int numBuckets = 10;
            const Vec3 step = maxDist / static_cast<float>(numBuckets);
            const float stepAxis = step[longestAxis];
            const float startBox = sur.pointMin[longestAxis];
            const float bucket1MaxLimit = startBox + stepAxis;
            auto itEnd = bn.begin() + end;
            auto itBucket = libstdcxxPartition(bn.begin() + begin, itEnd, [&](const BuildNode& node) {
                return node.centroid[longestAxis] < bucket1MaxLimit;
            });
            for (int32_t bucketIndex = 2; bucketIndex < numBuckets; ++bucketIndex) {
                const float bucketMaxLimit = startBox + stepAxis * bucketIndex;
                itBucket = libstdcxxPartition(itBucket, itEnd, [&](const BuildNode& node) {
                    return node.centroid[longestAxis] < bucketMaxLimit;
                });
            }
            Node& node = boxes[static_cast<size_t>(current)];
            node.box = bn[static_cast<size_t>(begin)].box;
            std::vector<AABB> bxs{node.box};
            for (int32_t i = begin + 1; i < end; ++i) {
                const AABB newBox = bn[static_cast<size_t>(i)].box;
                node.box = surroundingBox(newBox, node.box);
                bxs.push_back(newBox);
            }
            const int32_t count = end - begin;
            if (count <= 4) {
                node.indexOffset = begin;
                node.numPrimitives = count;
                current = stIdx.back();
                begin = stBegin.back();
                end = stEnd.back();
                stIdx.pop_back();
                stBegin.pop_back();
                stEnd.pop_back();
            } else {
                const int32_t left = maxNodeIndex + 1;
                const int32_t right = left + 1;
                const int32_t splitIndex = splitIndexSah(bxs);
                node.indexOffset = left;
                maxNodeIndex = std::max(right, maxNodeIndex);
                stIdx.push_back(right);
                stBegin.push_back(begin + splitIndex);
                stEnd.push_back(end);
                current = left;
                end = begin + splitIndex;
            }
        } while (!stIdx.empty());
        boxes.resize(static_cast<size_t>(maxNodeIndex + 1));
        primitives.reserve(n);
        for (size_t i = 0; i < n; ++i) primitives.push_back(prims[static_cast<size_t>(bn[i].oldIndex)]);
    }

    Intersection intersect(Intersection intersection) const {  // BVH.hpp:327-384
        if (primitives.empty()) return intersection;
        int32_t boxIndex = 0;
        std::vector<int32_t> stack;
        stack.reserve(64);
        stack.push_back(0);  // stack[0] is the sentinel the reference starts above
        do {
            const Node& node = boxes[static_cast<size_t>(boxIndex)];
            if (node.box.intersect(intersection.ray)) {
                const int32_t numberPrimitives = node.numPrimitives;
                if (numberPrimitives > 0) {
                    for (int32_t i = 0; i < numberPrimitives; ++i) {
                        const T& primitive = primitives[static_cast<size_t>(node.indexOffset + i)];
                        const float lastDist = intersection.length;
                        intersection = primitive.intersect(intersection);
                        if (intersection.ray.shadowTrace && intersection.length < lastDist) return intersection;
                    }
                    boxIndex = stack.back();
                    stack.pop_back();
                } else {
                    const int32_t left = node.indexOffset;
                    const int32_t right = node.indexOffset + 1;
                    const bool traverseLeft = boxes[static_cast<size_t>(left)].box.intersect(intersection.ray);
                    const bool traverseRight = boxes[static_cast<size_t>(right)].box.intersect(intersection.ray);
                    if (!traverseLeft && !traverseRight) {
                        boxIndex = stack.back();
                        stack.pop_back();
                    } else {
                        boxIndex = traverseLeft ? left : right;
                        if (traverseLeft && traverseRight) stack.push_back(right);
                    }
                }
            } else {
                boxIndex = stack.back();
                stack.pop_back();
            }
        } while (!stack.empty());
        return intersection;
    }
};

// ---- RegularGrid (RegularGrid.hpp) ------------------------------------------------------
// The primitives' own box tests, used only to fill the grid.
// Triangle::intersect(const AABB&) (Triangle.cpp:142-229): an edge half-line crosses the box,
// or the box's min->max diagonal ray hits the triangle, or that diagonal is parallel to it.
inline bool gridEdgeHitsBox(const Vec3& orig, const Vec3& vec, const AABB& box) {  // :143-201
    Vec3 t1, t2;
    float tNear = std::numeric_limits<float>::min();
    float tFar = std::numeric_limits<float>::max();
    for (int a = 0; a < 3; ++a) {
        if (std::fabs(vec[a]) < std::numeric_limits<float>::epsilon()) {
            if ((orig[a] < box.pointMin[a]) || ((orig[a] + vec[a]) > box.pointMax[a])) return false;
        } else {
            t1[a] = (box.pointMin[a] - orig[a]) / vec[a];
            t2[a] = (box.pointMax[a] - orig[a]) / vec[a];
            if (t1[a] > t2[a]) std::swap(t1, t2);
            tNear = std::max(t1[a], tNear);
            tFar = std::min(t2[a], tFar);
            if ((tNear > tFar) || (tFar < 0)) return false;  // isNearFarInvalid (:132-134)
        }
    }
    return true;
}
inline bool boxIntersect(const Triangle& t, const AABB& box) {
    const Vec3 vec = box.pointMax - box.pointMin;
    const Ray ray(vec, box.pointMin, 1, false, nullptr, nullptr);
    const bool ab = gridEdgeHitsBox(t.pointA, t.AB, box);
    const bool ac = gridEdgeHitsBox(t.pointA, t.AC, box);
    const Vec3 pointB = t.pointA + t.AB;
    const Vec3 pointC = t.pointA + t.AC;
    const bool bc = gridEdgeHitsBox(pointB, pointC - pointB, box);
    Intersection it(ray);
    const float lastDist = it.length;
    it = t.intersect(it);
    const bool hitRay = it.length < lastDist;
    const bool inside = std::abs(dot(t.AB, cross(vec, t.AC))) < Epsilon;
    return ab || ac || bc || hitRay || inside;
}
inline float planeDistance(const Plane& p, const Vec3& q) {  // Plane.cpp:117-138
    const float d = p.normal[0] * -p.point[0] + p.normal[1] * -p.point[1] + p.normal[2] * -p.point[2];
    const float numerator = p.normal[0] * q[0] + p.normal[1] * q[1] + p.normal[2] * q[2] + d;
    const float denumerator = std::sqrt(p.normal[0] * p.normal[0] + p.normal[1] * p.normal[1] + p.normal[2] * p.normal[2]);
    return numerator / denumerator;
}
inline bool boxIntersect(const Plane& p, const AABB& box) {  // Plane.cpp:146-155
    const float distanceP = planeDistance(p, box.pointMax);
    const float distanceN = planeDistance(p, box.pointMin);
    return (distanceP <= 0 && distanceN >= 0) || (distanceP >= 0 && distanceN <= 0);
}
inline bool boxIntersect(const Sphere& s, const AABB& box) {  // Sphere.cpp:102-123
    float dmin = 0.0F;
    for (int a = 0; a < 3; ++a) {
        if (s.center[a] < box.pointMin[a]) {
            dmin = dmin + (s.center[a] - box.pointMin[a]) * (s.center[a] - box.pointMin[a]);
        } else if (s.center[a] > box.pointMax[a]) {
            dmin = dmin + (s.center[a] - box.pointMax[a]) * (s.center[a] - box.pointMax[a]);
        }
    }
    return dmin <= s.sqRadius;
}

// static_cast<int32_t>(float) as x86 cvttss2si evaluates it (NaN / out of range: INT32_MIN),
// spelled out so the oracle does not depend on the compiler's treatment of that UB
inline int32_t cvtt(float f) {
    return (f >= -2147483648.0F && f < 2147483648.0F) ? static_cast<int32_t>(f) : std::numeric_limits<int32_t>::min();
}

template <typename T>
struct RegularGrid {  // RegularGrid.hpp:23-101, gridSize 32 (Shader.cpp:57)
    std::vector<std::vector<const T*>> grid;
    std::vector<T> primitives;
    int32_t gridSize = 32;
    uint32_t gridShift = 0;
    AABB worldBoundaries;
    Vec3 cellSizeInverted, cellSize;

    static uint32_t bitCounter(uint32_t value) {  // :173-180
        uint32_t counter = 0;
        while (value > 0) {
            ++counter;
            value >>= 1;
        }
        return counter;
    }

    RegularGrid(std::vector<T> prims, uint32_t size)  // :112-152
        : grid(static_cast<size_t>(size) * size * size), primitives(std::move(prims)),
          gridSize(static_cast<int32_t>(size)), gridShift(bitCounter(size - 1U)) {
        // Scene::getBounds (Scene.hpp:51-62)
        AABB bounds{Vec3(RayLengthMax), Vec3(-RayLengthMax)};
        for (const T& p : primitives) bounds = surroundingBox(p.getAABB(), bounds);
        worldBoundaries = AABB{bounds.pointMin - Vec3(Epsilon), bounds.pointMax + Vec3(Epsilon)};
        const Vec3 ext = worldBoundaries.pointMax - worldBoundaries.pointMin;
        cellSizeInverted = Vec3(static_cast<float>(gridSize) / ext[0], static_cast<float>(gridSize) / ext[1],
                                static_cast<float>(gridSize) / ext[2]);
        cellSize = ext * (1.0F / static_cast<float>(gridSize));
        addPrimitives();
    }

    // addPrimitivesThreadWork (:216-289) on one thread: every cell list in input order (the
    // reference's threads append under per-cell mutexes, in lock order)
    void addPrimitives() {
        const Vec3 worldBoundsMin = worldBoundaries.pointMin;
        const Vec3 size = worldBoundaries.pointMax - worldBoundsMin;
        const float dx = size[0] / gridSize, dy = size[1] / gridSize, dz = size[2] / gridSize;
        const float dxReci = dx > 0 ? 1.0F / dx : 1.0F;
        const float dyReci = dy > 0 ? 1.0F / dy : 1.0F;
        const float dzReci = dz > 0 ? 1.0F / dz : 1.0F;
        auto range = [&](float lo, float hi, float wmin, float sz, float reci, int32_t* a, int32_t* b) {
            int32_t v1 = cvtt((lo - wmin) * reci);
            int32_t v2 = cvtt((hi - wmin) * reci) + 1;
            v1 = std::max(0, v1);
            v2 = std::min(v2, gridSize - 1);
            v2 = std::fabs(sz) < std::numeric_limits<float>::epsilon() ? 0 : v2;
            v1 = std::min(v1, v2);
            *a = v1;
            *b = v2;
        };
        for (const T& primitive : primitives) {
            const AABB bound = primitive.getAABB();
            int32_t x1, x2, y1, y2, z1, z2;
            range(bound.pointMin[0], bound.pointMax[0], worldBoundsMin[0], size[0], dxReci, &x1, &x2);
            range(bound.pointMin[1], bound.pointMax[1], worldBoundsMin[1], size[1], dyReci, &y1, &y2);
            range(bound.pointMin[2], bound.pointMax[2], worldBoundsMin[2], size[2], dzReci, &z1, &z2);
            for (int32_t x = x1; x <= x2; ++x) {
                for (int32_t y = y1; y <= y2; ++y) {
                    for (int32_t z = z1; z <= z2; ++z) {
                        const uint32_t idx = static_cast<uint32_t>(x + y * gridSize + z * gridSize * gridSize);
                        const Vec3 pos(worldBoundsMin[0] + static_cast<float>(x) * dx,
                                       worldBoundsMin[1] + static_cast<float>(y) * dy,
                                       worldBoundsMin[2] + static_cast<float>(z) * dz);
                        const AABB cell{pos, pos + Vec3(dx, dy, dz)};
                        if (boxIntersect(primitive, cell)) grid[idx].push_back(&primitive);
                    }
                }
            }
        }
    }

    int32_t cellIndex(int32_t x, int32_t y, int32_t z) const {  // getCellIndex (:526-538)
        return static_cast<int32_t>(static_cast<uint32_t>(x) + (static_cast<uint32_t>(y) << gridShift) +
                                    (static_cast<uint32_t>(z) << (gridShift * 2U)));
    }

    Intersection intersect(Intersection intersection) const {  // :333-515
        const Vec3 worldBoundsMin = worldBoundaries.pointMin;
        const Vec3 cell = (intersection.ray.origin - worldBoundsMin) * cellSizeInverted;
        int32_t cellX = cvtt(cell[0]), cellY = cvtt(cell[1]), cellZ = cvtt(cell[2]);
        cellX = std::max(std::min(cellX, gridSize - 1), 0);
        cellY = std::max(std::min(cellY, gridSize - 1), 0);
        cellZ = std::max(std::min(cellZ, gridSize - 1), 0);
        int32_t stepX, outX, stepY, outY, stepZ, outZ;
        Vec3 cb;
        const Vec3& dir = intersection.ray.direction;
        const Vec3& org = intersection.ray.origin;
        if (dir[0] > 0) { stepX = 1; outX = gridSize; cb[0] = worldBoundsMin[0] + (static_cast<float>(cellX) + 1.0F) * cellSize[0]; }
        else { stepX = -1; outX = -1; cb[0] = worldBoundsMin[0] + static_cast<float>(cellX) * cellSize[0]; }
        if (dir[1] > 0) { stepY = 1; outY = gridSize; cb[1] = worldBoundsMin[1] + (static_cast<float>(cellY) + 1.0F) * cellSize[1]; }
        else { stepY = -1; outY = -1; cb[1] = worldBoundsMin[1] + static_cast<float>(cellY) * cellSize[1]; }
        if (dir[2] > 0) { stepZ = 1; outZ = gridSize; cb[2] = worldBoundsMin[2] + (static_cast<float>(cellZ) + 1.0F) * cellSize[2]; }
        else { stepZ = -1; outZ = -1; cb[2] = worldBoundsMin[2] + static_cast<float>(cellZ) * cellSize[2]; }
        Vec3 tmax, tdelta;
        const float eps = std::numeric_limits<float>::epsilon();
        if (std::fabs(dir[0]) > eps) { const float r = 1.0F / dir[0]; tmax[0] = (cb[0] - org[0]) * r; tdelta[0] = cellSize[0] * static_cast<float>(stepX) * r; }
        else { tmax[0] = RayLengthMax; }
        if (std::fabs(dir[1]) > eps) { const float r = 1.0F / dir[1]; tmax[1] = (cb[1] - org[1]) * r; tdelta[1] = cellSize[1] * static_cast<float>(stepY) * r; }
        else { tmax[1] = RayLengthMax; }
        if (std::fabs(dir[2]) > eps) { const float r = 1.0F / dir[2]; tmax[2] = (cb[2] - org[2]) * r; tdelta[2] = cellSize[2] * static_cast<float>(stepZ) * r; }
        else { tmax[2] = RayLengthMax; }
        // first loop: until a primitive of this grid improves the hit (shadow rays return there)
        while (true) {
            for (const T* primitive : grid[static_cast<size_t>(cellIndex(cellX, cellY, cellZ))]) {
                const float lastDist = intersection.length;
                intersection = primitive->intersect(intersection);
                if (intersection.length < lastDist) {
                    if (intersection.ray.shadowTrace) return intersection;
                    goto testloop;
                }
            }
            if (tmax[0] < tmax[1]) {
                if (tmax[0] < tmax[2]) { cellX += stepX; if (cellX == outX) return intersection; tmax[0] = tmax[0] + tdelta[0]; }
                else { cellZ += stepZ; if (cellZ == outZ) return intersection; tmax[2] = tmax[2] + tdelta[2]; }
            } else {
                if (tmax[1] < tmax[2]) { cellY += stepY; if (cellY == outY) return intersection; tmax[1] = tmax[1] + tdelta[1]; }
                else { cellZ += stepZ; if (cellZ == outZ) return intersection; tmax[2] = tmax[2] + tdelta[2]; }
            }
        }
    testloop:
        while (true) {
            for (const T* primitive : grid[static_cast<size_t>(cellIndex(cellX, cellY, cellZ))])
                intersection = primitive->intersect(intersection);
            if (tmax[0] < tmax[1]) {
                if (tmax[0] < tmax[2]) {
                    if (intersection.length < tmax[0]) break;
                    cellX += stepX; if (cellX == outX) break; tmax[0] = tmax[0] + tdelta[0];
                } else {
                    if (intersection.length < tmax[2]) break;
                    cellZ += stepZ; if (cellZ == outZ) break; tmax[2] = tmax[2] + tdelta[2];
                }
            } else {
                if (tmax[1] < tmax[2]) {
                    if (intersection.length < tmax[1]) break;
                    cellY += stepY; if (cellY == outY) break; tmax[1] = tmax[1] + tdelta[1];
                } else {
                    if (intersection.length < tmax[2]) break;
                    cellZ += stepZ; if (cellZ == outZ) break; tmax[2] = tmax[2] + tdelta[2];
                }
            }
        }
        return intersection;
    }
};

// ---- lights -------------------------------------------------------------------------------
struct Light {
    Material radiance;
    bool area = false;
    Vec3 position;       // point light
    Triangle triangle{}; // area light
    int64_t index = -1;
};

// ---- camera -------------------------------------------------------------------------------
struct Camera {  // Camera.cpp:14-19, Perspective.cpp, Orthographic.cpp
    Vec3 position, direction, right, up;
    float hFov = 0, vFov = 0;
    bool ortho = false;
    float sizeH = 0, sizeV = 0;  // Orthographic: half sizes (Orthographic.cpp:8-13)
    static Camera orthographic(const Vec3& pos, const Vec3& lookAt, const Vec3& upv, float sH, float sV) {
        Camera c;
        c.position = pos;
        c.direction = normalize(lookAt - pos);
        c.right = cross(upv, c.direction);
        c.up = cross(c.direction, c.right);
        c.ortho = true;
        c.sizeH = sH / 2.0F;
        c.sizeV = sV / 2.0F;
        return c;
    }
    static float degToRad(float deg) { return (deg * kPi) / 180.0F; }
    static Camera perspective(const Vec3& pos, const Vec3& lookAt, const Vec3& upv, float hFovDeg, float vFovDeg) {
        Camera c;
        c.position = pos;
        c.direction = normalize(lookAt - pos);
        c.right = cross(upv, c.direction);
        c.up = cross(c.direction, c.right);
        c.hFov = degToRad(hFovDeg);
        c.vFov = degToRad(vFovDeg);
        return c;
    }
    static float fastArcTan(float value) {  // Perspective.cpp:40-46
        const float absValue = std::abs(value);
        return kQuarterPi * value - (value * (absValue - 1.0F)) * (0.2447F + (0.0663F * absValue));
    }
    Ray generateRay(float u, float v, float du, float dv, std::atomic<uint64_t>* counter) const {
        if (ortho) {  // Orthographic.cpp:15-24
            const float rightFactor = (u - 0.5F) * sizeH;
            const Vec3 r = right * rightFactor + right * du;
            const float upFactor = (0.5F - v) * sizeV;
            const Vec3 uu = up * upFactor + up * dv;
            return Ray(direction, position + r + uu, 1, false, nullptr, counter);
        }
        const float rightFactor = fastArcTan(hFov * (u - 0.5F)) + du;
        const Vec3 r = right * rightFactor;
        const float upFactor = fastArcTan(vFov * (0.5F - v)) + dv;
        const Vec3 uu = up * upFactor;
        const Vec3 dest = position + direction + r + uu;
        return Ray(normalize(dest - position), position, 1, false, nullptr, counter);
    }
};

// ---- scene + loaders ------------------------------------------------------------------------
struct Scene {
    std::vector<Triangle> triangles;
    std::vector<Plane> planes;
    std::vector<Sphere> spheres;
    std::vector<Light> lights;
    std::vector<Material> materials;
};

void cornellBoxWalls(Scene* s);

void cornellBox(Scene* s, Camera* cam, float ratio) {  // Scenes.cpp:19-150
    const Material lightMat(Vec3(0.0F), Vec3(0.0F), Vec3(0.0F), 1.0F, Vec3(0.9F, 0.9F, 0.9F));
    const Material mirrorMat(Vec3(0.0F), Vec3(0.9F, 0.9F, 0.9F), Vec3(0.0F), 1.0F);
    Light pl;
    pl.radiance = lightMat;
    pl.position = Vec3(0.0F, 0.99F, 0.0F);
    pl.index = 0;
    s->lights.push_back(pl);
    Triangle t = Triangle::build(Vec3(0.5F, -0.5F, 0.99F), Vec3(0.5F, 0.5F, 1.001F), Vec3(-0.5F, -0.5F, 0.99F), nullptr,
                                 nullptr, nullptr, static_cast<int32_t>(s->materials.size()));
    s->triangles.push_back(t);
    s->materials.emplace_back(Vec3(0.9F, 0.9F, 0.0F));
    s->spheres.emplace_back(Vec3(0.45F, -0.65F, 0.4F), 0.35F, static_cast<int32_t>(s->materials.size()));
    s->materials.push_back(mirrorMat);
    s->spheres.emplace_back(Vec3(-0.45F, -0.1F, 0.0F), 0.35F, static_cast<int32_t>(s->materials.size()));
    s->materials.emplace_back(Vec3(0.0F, 0.9F, 0.0F));
    cornellBoxWalls(s);
    *cam = Camera::perspective(Vec3(0.0F, 0.0F, -3.4F), Vec3(0.0F, 0.0F, 1.0F), Vec3(0.0F, 1.0F, 0.0F), 45.0F * ratio, 45.0F);
}

void cornellBoxWalls(Scene* s) {  // Scenes.cpp:63-107
    const Material gray(Vec3(0.7F, 0.7F, 0.7F));
    struct P { Vec3 p, n; Material m; };
    const P ps[] = {{Vec3(0, 0, 1), Vec3(0, 0, -1), gray},
                    {Vec3(0, 0, -3.5F), Vec3(0, 0, 1), Material(Vec3(0.0F, 0.9F, 0.9F))},
                    {Vec3(0, -1, 0), Vec3(0, 1, 0), gray},
                    {Vec3(0, 1, 0), Vec3(0, -1, 0), gray},
                    {Vec3(-1, 0, 0), Vec3(1, 0, 0), Material(Vec3(0.9F, 0.0F, 0.0F))},
                    {Vec3(1, 0, 0), Vec3(-1, 0, 0), Material(Vec3(0.0F, 0.0F, 0.9F))}};
    for (const P& p : ps) {
        s->planes.emplace_back(p.p, p.n, static_cast<int32_t>(s->materials.size()));
        s->materials.push_back(p.m);
    }
}

// Scenes.cpp:152-224 (scene 2: two area lights, transmission sphere)
void cornellBox2(Scene* s, Camera* cam, float ratio) {
    const Material lightMat(Vec3(0.0F), Vec3(0.0F), Vec3(0.0F), 1.0F, Vec3(0.9F, 0.9F, 0.9F));
    const Material mirrorMat(Vec3(0.0F), Vec3(0.9F, 0.9F, 0.9F), Vec3(0.0F), 1.0F);
    const Material transmissionMat(Vec3(0.0F), Vec3(0.0F), Vec3(0.9F, 0.9F, 0.9F), 1.9F);
    const Vec3 quad[2][3] = {{Vec3(-0.25F, 0.99F, -0.25F), Vec3(0.25F, 0.99F, -0.25F), Vec3(0.25F, 0.99F, 0.25F)},
                             {Vec3(0.25F, 0.99F, 0.25F), Vec3(-0.25F, 0.99F, 0.25F), Vec3(-0.25F, 0.99F, -0.25F)}};
    for (const auto& q : quad) {
        Light l;
        l.area = true;
        l.radiance = lightMat;
        l.triangle = Triangle::build(q[0], q[1], q[2], nullptr, nullptr, nullptr, -1);
        l.index = static_cast<int64_t>(s->lights.size());
        s->lights.push_back(l);
    }
    s->triangles.push_back(Triangle::build(Vec3(0.5F, -0.5F, 0.99F), Vec3(0.5F, 0.5F, 1.001F), Vec3(-0.5F, -0.5F, 0.99F),
                                           nullptr, nullptr, nullptr, static_cast<int32_t>(s->materials.size())));
    s->materials.emplace_back(Vec3(0.9F, 0.9F, 0.0F));
    s->triangles.push_back(Triangle::build(Vec3(-0.5F, 0.5F, 0.99F), Vec3(-0.5F, -0.5F, 0.99F), Vec3(0.5F, 0.5F, 0.99F),
                                           nullptr, nullptr, nullptr, static_cast<int32_t>(s->materials.size())));
    s->materials.emplace_back(Vec3(0.0F, 0.9F, 0.0F));
    s->spheres.emplace_back(Vec3(0.45F, -0.65F, 0.4F), 0.35F, static_cast<int32_t>(s->materials.size()));
    s->materials.push_back(mirrorMat);
    s->spheres.emplace_back(Vec3(-0.4F, -0.3F, 0.0F), 0.35F, static_cast<int32_t>(s->materials.size()));
    s->materials.push_back(transmissionMat);
    cornellBoxWalls(s);
    *cam = Camera::perspective(Vec3(0.0F, 0.0F, -3.4F), Vec3(0.0F, 0.0F, 1.0F), Vec3(0.0F, 1.0F, 0.0F), 45.0F * ratio, 45.0F);
}

// Scenes.cpp:227-262 (scene 1: no lights, orthographic camera)
void spheres(Scene* s, Camera* cam, float ratio) {
    s->spheres.emplace_back(Vec3(4.0F, 4.0F, 4.0F), 4.0F, static_cast<int32_t>(s->materials.size()));
    s->materials.emplace_back(Vec3(0.9F, 0.0F, 0.0F));
    s->triangles.push_back(Triangle::build(Vec3(0.0F, 10.0F, 10.0F), Vec3(0.0F, 0.0F, 10.0F), Vec3(10.0F, 0.0F, 10.0F),
                                           nullptr, nullptr, nullptr, static_cast<int32_t>(s->materials.size())));
    s->materials.emplace_back(Vec3(0.914F, 0.723F, 0.531F));
    *cam = Camera::orthographic(Vec3(0.0F, 1.0F, -10.0F), Vec3(0.0F, 1.0F, 7.0F), Vec3(0.0F, 1.0F, 0.0F), 10.0F * ratio,
                                10.0F);
}

// Scenes.cpp:264-302 (scene 3: point light, five spheres, a floor plane)
void spheres2(Scene* s, Camera* cam, float ratio) {
    Light pl;
    pl.radiance = Material(Vec3(0.0F), Vec3(0.0F), Vec3(0.0F), 1.0F, Vec3(0.9F, 0.9F, 0.9F));
    pl.position = Vec3(0.0F, 15.0F, 4.0F);
    pl.index = 0;
    s->lights.push_back(pl);
    const Material mirrorMat(Vec3(0.0F), Vec3(0.9F, 0.9F, 0.9F), Vec3(0.0F), 1.0F);
    struct Sp { Vec3 c; float r; Material m; };
    const Sp sp[] = {{Vec3(-1.0F, 1.0F, 6.0F), 1.0F, Material(Vec3(0.9F, 0.0F, 0.0F))},
                     {Vec3(-0.5F, 2.0F, 5.0F), 0.3F, Material(Vec3(0.0F, 0.0F, 0.9F))},
                     {Vec3(0.0F, 2.0F, 7.0F), 1.0F, mirrorMat},
                     {Vec3(0.5F, 0.5F, 5.0F), 0.2F, Material(Vec3(0.9F, 0.9F, 0.0F))},
                     {Vec3(1.0F, 0.5F, 4.5F), 0.5F, Material(Vec3(0.0F, 0.9F, 0.0F))}};
    for (const Sp& q : sp) {
        s->spheres.emplace_back(q.c, q.r, static_cast<int32_t>(s->materials.size()));
        s->materials.push_back(q.m);
    }
    s->planes.emplace_back(Vec3(0.0F, 0.0F, 0.0F), Vec3(0.0F, 1.0F, 0.0F), static_cast<int32_t>(s->materials.size()));
    s->materials.emplace_back(Vec3(0.914F, 0.723F, 0.531F));
    *cam = Camera::perspective(Vec3(0.0F, 0.5F, 1.0F), Vec3(0.0F, 0.0F, 7.0F), Vec3(0.0F, 1.0F, 0.0F), 60.0F * ratio, 60.0F);
}

// tinyobjloader v1.0.7 number parser
bool tinyobjParseDouble(const char* s, const char* s_end, double* result) {
    if (s >= s_end) return false;
    double mantissa = 0.0;
    int exponent = 0;
    char sign = '+', exp_sign = '+';
    char const* curr = s;
    int read = 0;
    bool end_not_reached = false;
    if (*curr == '+' || *curr == '-') {
        sign = *curr;
        curr++;
    } else if (*curr >= '0' && *curr <= '9') {
    } else if (*curr == '.') {
    } else {
        return false;
    }
    end_not_reached = (curr != s_end);
    while (end_not_reached && (*curr >= '0' && *curr <= '9')) {
        mantissa *= 10;
        mantissa += static_cast<int>(*curr - 0x30);
        curr++;
        read++;
        end_not_reached = (curr != s_end);
    }
    if (!end_not_reached) goto assemble;
    if (*curr == '.') {
        curr++;
        read = 1;
        end_not_reached = (curr != s_end);
        while (end_not_reached && (*curr >= '0' && *curr <= '9')) {
            static const double pow_lut[] = {1.0, 0.1, 0.01, 0.001, 0.0001, 0.00001, 0.000001, 0.0000001};
            const int lut_entries = sizeof pow_lut / sizeof pow_lut[0];
            mantissa += static_cast<int>(*curr - 0x30) * (read < lut_entries ? pow_lut[read] : std::pow(10.0, -read));
            read++;
            curr++;
            end_not_reached = (curr != s_end);
        }
    } else if (*curr == 'e' || *curr == 'E') {
    } else {
        goto assemble;
    }
    if (!end_not_reached) goto assemble;
    if (*curr == 'e' || *curr == 'E') {
        curr++;
        end_not_reached = (curr != s_end);
        if (end_not_reached && (*curr == '+' || *curr == '-')) {
            exp_sign = *curr;
            curr++;
        } else if (end_not_reached && (*curr >= '0' && *curr <= '9')) {
        } else {
            return false;
        }
        read = 0;
        end_not_reached = (curr != s_end);
        while (end_not_reached && (*curr >= '0' && *curr <= '9')) {
            exponent *= 10;
            exponent += static_cast<int>(*curr - 0x30);
            curr++;
            read++;
            end_not_reached = (curr != s_end);
        }
        exponent *= (exp_sign == '+' ? 1 : -1);
        if (read == 0) return false;
    }
assemble:
    *result = (sign == '+' ? 1 : -1) * (exponent ? std::ldexp(mantissa * std::pow(5.0, exponent), exponent) : mantissa);
    return true;
}

struct Tok {
    const char* p;
    void skip() { while (*p == ' ' || *p == '\t') ++p; }
    float real(double def = 0.0) {
        skip();
        const char* e = p;
        while (*e && *e != ' ' && *e != '\t' && *e != '\r' && *e != '\n') ++e;
        double v = def;
        tinyobjParseDouble(p, e, &v);
        p = e;
        return static_cast<float>(v);
    }
};

struct MtlEntry {
    float kd[3] = {0, 0, 0}, ks[3] = {0, 0, 0}, tf[3] = {0, 0, 0}, ke[3] = {0, 0, 0};
    float ior = 1.0F, dissolve = 1.0F;
    std::string mapKd;
};

bool startsKey(const char* t, const char* key) {
    const size_t n = std::strlen(key);
    return std::strncmp(t, key, n) == 0 && (t[n] == ' ' || t[n] == '\t');
}

bool loadObj(const std::string& objPath, const std::string& mtlPath, Scene* scene, std::string* err) {
    std::vector<MtlEntry> mats;
    std::unordered_map<std::string, int> names;
    {
        std::ifstream in(mtlPath);
        std::string line, current;
        MtlEntry m;
        bool have = false, hasD = false;
        while (std::getline(in, line)) {
            while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
            Tok t{line.c_str()};
            t.skip();
            if (*t.p == 0 || *t.p == '#') continue;
            if (startsKey(t.p, "newmtl")) {
                if (have) {
                    names[current] = static_cast<int>(mats.size());
                    mats.push_back(m);
                }
                m = MtlEntry();
                hasD = false;
                t.p += 6;
                t.skip();
                current = t.p;
                have = true;
            } else if (startsKey(t.p, "Kd")) { t.p += 2; for (float& c : m.kd) c = t.real(); }
            else if (startsKey(t.p, "Ks")) { t.p += 2; for (float& c : m.ks) c = t.real(); }
            else if (startsKey(t.p, "Kt") || startsKey(t.p, "Tf")) { t.p += 2; for (float& c : m.tf) c = t.real(); }
            else if (startsKey(t.p, "Ke")) { t.p += 2; for (float& c : m.ke) c = t.real(); }
            else if (startsKey(t.p, "Ni")) { t.p += 2; m.ior = t.real(); }
            else if (startsKey(t.p, "d")) { t.p += 1; m.dissolve = t.real(); hasD = true; }
            else if (startsKey(t.p, "Tr")) { t.p += 2; const float v = t.real(); if (!hasD) m.dissolve = 1.0F - v; }
            else if (startsKey(t.p, "map_Kd")) {
                t.p += 6;
                t.skip();
                m.mapKd = t.p;
                while (!m.mapKd.empty() && (m.mapKd.back() == ' ' || m.mapKd.back() == '\t')) m.mapKd.pop_back();
            }
        }
        if (have) {
            names[current] = static_cast<int>(mats.size());
            mats.push_back(m);
        }
    }
    std::ifstream in(objPath);
    if (!in) {
        *err = "cannot open " + objPath;
        return false;
    }
    std::vector<float> vs, vn, vt, cols;
    std::string line;
    int material = -1;
    int64_t faceCounter = 0;
    struct Idx { int v, n, t; };
    std::vector<Idx> face;
    std::vector<std::array<Idx, 3>> tris;
    std::vector<int> triMat;
    while (std::getline(in, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
        Tok t{line.c_str()};
        t.skip();
        const char* p = t.p;
        if (p[0] == 'v' && (p[1] == ' ' || p[1] == '\t')) {
            t.p += 1;
            const float x = t.real(), y = t.real(), z = t.real();
            const float r = t.real(1.0), g = t.real(1.0), b = t.real(1.0);
            vs.insert(vs.end(), {x, y, z});
            cols.insert(cols.end(), {r, g, b});
        } else if (p[0] == 'v' && p[1] == 'n' && (p[2] == ' ' || p[2] == '\t')) {
            t.p += 2;
            const float x = t.real(), y = t.real(), z = t.real();
            vn.insert(vn.end(), {x, y, z});
        } else if (p[0] == 'v' && p[1] == 't' && (p[2] == ' ' || p[2] == '\t')) {
            t.p += 2;
            const float u = t.real(), v = t.real();
            vt.insert(vt.end(), {u, v});
        } else if (p[0] == 'f' && (p[1] == ' ' || p[1] == '\t')) {
            face.clear();
            const char* q = p + 2;
            const int nv = static_cast<int>(vs.size() / 3), nn = static_cast<int>(vn.size() / 3),
                      nt = static_cast<int>(vt.size() / 2);
            auto fix = [](int i, int n) { return i > 0 ? i - 1 : (i == 0 ? 0 : n + i); };
            while (true) {
                while (*q == ' ' || *q == '\t') ++q;
                if (*q == 0) break;
                Idx id{fix(std::atoi(q), nv), -1, -1};
                while (*q && *q != '/' && *q != ' ' && *q != '\t') ++q;
                if (*q == '/') {
                    ++q;
                    if (*q != '/') {  // texcoord
                        id.t = fix(std::atoi(q), nt);
                        while (*q && *q != '/' && *q != ' ' && *q != '\t') ++q;
                    }
                    if (*q == '/') {
                        ++q;
                        id.n = fix(std::atoi(q), nn);
                        while (*q && *q != ' ' && *q != '\t') ++q;
                    }
                }
                face.push_back(id);
            }
            for (size_t k = 2; k < face.size(); ++k) {  // tinyobjloader 1.0.7 fan triangulation
                tris.push_back({face[0], face[k - 1], face[k]});
                triMat.push_back(material);
            }
            ++faceCounter;
        } else if (startsKey(p, "usemtl")) {
            std::string nm(p + 7);
            while (!nm.empty() && (nm.front() == ' ' || nm.front() == '\t')) nm.erase(nm.begin());
            while (!nm.empty() && (nm.back() == ' ' || nm.back() == '\t')) nm.pop_back();
            auto it = names.find(nm);
            material = it == names.end() ? -1 : it->second;
        }
    }
    const bool hasNormals = !vn.empty();
    for (size_t k = 0; k < tris.size(); ++k) {  // OBJLoader.cpp:276-497, single thread, file order
        const auto& f = tris[k];
        Vec3 v[3], n[3];
        for (int j = 0; j < 3; ++j) {
            const int i = f[static_cast<size_t>(j)].v;
            v[j] = Vec3(-vs[3 * i], vs[3 * i + 1], vs[3 * i + 2]);
        }
        if (hasNormals && f[0].n >= 0 && f[1].n >= 0 && f[2].n >= 0) {
            for (int j = 0; j < 3; ++j) {
                const int i = f[static_cast<size_t>(j)].n;
                n[j] = Vec3(-vn[3 * i], vn[3 * i + 1], vn[3 * i + 2]);
            }
        } else {
            const Vec3 AB = v[1] - v[0], AC = v[2] - v[0];
            n[0] = n[1] = n[2] = normalize(cross(AC, AB));
        }
        const int mid = triMat[k];
        Material mat;
        Vec2 tcs[3] = {Vec2{-1.0F, -1.0F}, Vec2{-1.0F, -1.0F}, Vec2{-1.0F, -1.0F}};
        if (mid >= 0) {
            const MtlEntry& e = mats[static_cast<size_t>(mid)];
            Vec3 emission(e.ke[0], e.ke[1], e.ke[2]);
            const float mx = std::max(std::max(emission[0], emission[1]), emission[2]);
            if (mx > 1.0F) emission = emission / mx;  // Utils.cpp:189-196
            mat = Material(Vec3(e.kd[0], e.kd[1], e.kd[2]), Vec3(e.ks[0], e.ks[1], e.ks[2]),
                           Vec3(e.tf[0], e.tf[1], e.tf[2]) * (1.0F - e.dissolve), e.ior, emission);
            // OBJLoader.cpp:332-364: texture + coordinates wrapped into [0, 1) (glm::fract)
            if (!e.mapKd.empty() && !vt.empty()) {
                const std::string dir = objPath.find('/') == std::string::npos ? "" : objPath.substr(0, objPath.rfind('/') + 1);
                auto it = textureRegistry().find(dir + e.mapKd);
                if (it != textureRegistry().end()) {
                    mat.texture = e.mapKd;
                    mat.tex = &it->second;
                    if (f[0].t >= 0 && f[1].t >= 0 && f[2].t >= 0) {
                        auto fr = [](float x) { return x - std::floor(x); };
                        for (int j = 0; j < 3; ++j) {
                            const int ti = f[static_cast<size_t>(j)].t;
                            tcs[j] = Vec2{fr(vt[2 * static_cast<size_t>(ti)]), fr(vt[2 * static_cast<size_t>(ti) + 1])};
                        }
                    }
                }
            }
            if (hasPositiveValue(emission)) {
                Light l;
                l.area = true;
                l.radiance = mat;
                l.triangle = Triangle::build(v[0], v[1], v[2], &n[0], &n[1], &n[2], -1);
                l.index = static_cast<int64_t>(scene->lights.size());
                scene->lights.push_back(l);
                continue;
            }
        } else {
            const int i = f[0].v;
            mat = Material(Vec3(cols[3 * i], cols[3 * i + 1], cols[3 * i + 2]));
        }
        const auto it = std::find(scene->materials.begin(), scene->materials.end(), mat);
        int32_t mi;
        if (it != scene->materials.end()) {
            mi = static_cast<int32_t>(it - scene->materials.begin());
        } else {
            mi = static_cast<int32_t>(scene->materials.size());
            scene->materials.push_back(mat);
        }
        Triangle tri = Triangle::build(v[0], v[1], v[2], &n[0], &n[1], &n[2], mi);
        tri.texA = tcs[0];
        tri.texB = tcs[1];
        tri.texC = tcs[2];
        scene->triangles.push_back(tri);
    }
    return true;
}

bool loadCamera(const std::string& path, float ratio, Camera* cam) {  // CameraFactory.cpp, PerspectiveLoader.cpp
    std::ifstream in(path);
    std::string line;
    bool found = false;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == 't' && line.find("perspective") != std::string::npos) {
            found = true;
            break;
        }
    }
    if (!found) return false;
    Vec3 position, lookAt, up;
    float fov[2] = {0, 0};
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        const char key = line[0];
        std::stringstream data(line.substr(1));
        if (key == 'p') data >> position[0] >> position[1] >> position[2];
        else if (key == 'l') data >> lookAt[0] >> lookAt[1] >> lookAt[2];
        else if (key == 'u') data >> up[0] >> up[1] >> up[2];
        else if (key == 'f') data >> fov[0] >> fov[1];
    }
    position[0] = -position[0];
    *cam = Camera::perspective(position, lookAt, up, fov[0] * ratio, fov[1]);
    return true;
}

// ---- shader + renderer ---------------------------------------------------------------------
struct Config {
    int32_t width, height, shader, sceneIndex, samplesPixel, samplesLight, maxDepth;
    const char* obj;
    const char* mtl;
    const char* cam;
    int32_t accelerator;  // Shader::Accelerator (Shader.hpp:20-24)
};

struct Engine {
    Config cfg{};
    Camera camera;
    Vec3 maxPoint;  // DepthMap (C_wrapper.cpp:79-131)
    std::vector<Material> materials;
    std::vector<Light> lights;
    std::unique_ptr<BVH<Plane>> planes;
    std::unique_ptr<BVH<Sphere>> spheres;
    std::unique_ptr<BVH<Triangle>> triangles;
    std::unique_ptr<RegularGrid<Plane>> gridPlanes;  // RegularGrid accelerator (Shader.cpp:56-61)
    std::unique_ptr<RegularGrid<Sphere>> gridSpheres;
    std::unique_ptr<RegularGrid<Triangle>> gridTriangles;
    std::vector<Plane> naivePlanes;  // input order (Naive accelerator)
    std::vector<Sphere> naiveSpheres;
    std::vector<Triangle> naiveTriangles;
    std::vector<float> shaderTable, samplerTable;
    std::atomic<uint64_t> rays{0};
    int64_t numTriangles = 0;
    // Timing-faithful mode (bench.py cpu_baseline): draws come from the
    // reference's shared atomic cursors instead of the deterministic index - the hemisphere's
    // (Shader.cpp:189-194, two per call) and the light index's (:224-227) static cursors, and the
    // per-instance cursors of the StaticHaltonSeq samplers (Sampler.hpp:58-63): the pixel sampler,
    // the PathTracer's Russian roulette, one per area light.  Results then depend on thread
    // scheduling, as the reference's do.
    bool faithful = false;
    float pixelValue = 0.5F;  // the Constant pixel sampler's value (C_wrapper.cpp:144-148: 0.5)
    mutable std::atomic<uint32_t> curHemi{0}, curLight{0}, curPixel{0}, curRR{0};
    mutable std::vector<std::atomic<uint32_t>> curArea = std::vector<std::atomic<uint32_t>>(64);
    uint32_t draw(uint32_t key, uint32_t tc, uint32_t purpose, std::atomic<uint32_t>& cursor) const {
        if (!faithful) return sampleIndex(key, tc, purpose);
        return cursor.fetch_add(1, std::memory_order_relaxed) & ArrayMask;
    }

    struct Ctx {
        uint32_t key;
        std::vector<Material>* mats;  // this thread's materials: rayTrace writes textured Kd (Shader.cpp:116-120)
    };

    Intersection traceLights(Intersection it) const {  // Shader.cpp:166-171
        for (const Light& l : lights) {
            if (!l.area) continue;  // PointLight::intersect returns the record unchanged
            const float lastDist = it.length;
            it = l.triangle.intersect(it);
            if (it.length < lastDist) {  // AreaLight.cpp:32-41
                it.material = &l.radiance;
                it.materialIndex = -1;
                it.kind = 4;
                it.index = l.index;
            }
        }
        return it;
    }

    // Naive<T>::intersect (Naive.hpp): every primitive in input order; a shadow ray returns at its
    // first hit closer than its distance
    template <class T>
    static Intersection naive(const std::vector<T>& prims, Intersection it) {
        const float lastDist = it.length;
        for (const T& p : prims) {
            it = p.intersect(it);
            if (it.ray.shadowTrace && it.length < lastDist) return it;
        }
        return it;
    }

    // Shader.cpp:88-110: the accelerator switch (an id other than 1-3 builds none: only lights hit)
    Intersection geometry(Intersection it) const {
        if (cfg.accelerator == 1) {
            it = naive(naivePlanes, it);
            it = naive(naiveSpheres, it);
            it = naive(naiveTriangles, it);
        } else if (cfg.accelerator == 2) {
            it = gridPlanes->intersect(it);
            it = gridSpheres->intersect(it);
            it = gridTriangles->intersect(it);
        } else if (cfg.accelerator == 3) {
            it = planes->intersect(it);
            it = spheres->intersect(it);
            it = triangles->intersect(it);
        }
        return it;
    }

    Intersection closest(Intersection it) const { return traceLights(geometry(it)); }

    // Shader::rayTrace (Shader.cpp:86-123); tc = vertex code in the ray tree
    bool rayTrace(Vec3* rgb, const Ray& ray, Ctx ctx, uint32_t tc) {
        Intersection it(ray);
        const float lastDist = it.length;
        it = closest(it);
        if (it.materialIndex >= 0) {  // Shader.cpp:112-121
            Material& material = (*ctx.mats)[static_cast<size_t>(it.materialIndex)];
            it.material = &material;
            if (it.texCoords.x >= 0 && it.texCoords.y >= 0 && material.tex != nullptr)
                material.Kd = material.tex->loadColor(it.texCoords);
        }
        return it.length < lastDist && shade(rgb, it, ctx, tc);
    }

    // Shader::shadowTrace (Shader.cpp:132-158)
    bool shadowTrace(float distance, const Ray& ray) const {
        Intersection it(ray, distance);
        it = geometry(it);
        return it.length < distance;
    }

    Vec3 cosineSampleHemisphere(const Vec3& normal, Ctx ctx, uint32_t tc) const {  // Shader.cpp:188-216
        const float uniformRandom1 = shaderTable[draw(ctx.key, tc, P_HEMI1, curHemi)];
        const float uniformRandom2 = shaderTable[draw(ctx.key, tc, P_HEMI2, curHemi)];
        float cosPhi, sinPhi;
        hemisphereTrig(uniformRandom1, &cosPhi, &sinPhi);  // std::cos(phi), std::sin(phi), phi = 2 pi r1
        const float r2 = uniformRandom2;
        const float cosTheta = std::sqrt(r2);
        Vec3 u = std::abs(normal[0]) > 0.1F ? Vec3(0.0F, 1.0F, 0.0F) : Vec3(1.0F, 0.0F, 0.0F);
        u = normalize(cross(u, normal));
        const Vec3 v = cross(normal, u);
        Vec3 direction = u * (cosPhi * cosTheta) + v * (sinPhi * cosTheta) + normal * std::sqrt(1.0F - r2);
        return normalize(direction);
    }

    uint32_t lightIndex(Ctx ctx, uint32_t tc, int i) const {  // Shader.cpp:223-233
        const float randomNumber = shaderTable[draw(ctx.key, tc, P_LIGHT + 3u * static_cast<uint32_t>(i), curLight)];
        const uint32_t sizeLights = static_cast<uint32_t>(lights.size());
        return static_cast<uint32_t>(std::floor(randomNumber * sizeLights * 0.99999F));
    }

    Vec3 lightPosition(const Light& l, Ctx ctx, uint32_t tc, int i) const {  // AreaLight.cpp:17-26
        if (!l.area) return l.position;
        std::atomic<uint32_t>& cur = curArea[static_cast<size_t>(l.index) & 63u];
        float r = samplerTable[draw(ctx.key, tc, P_LIGHT + 3u * static_cast<uint32_t>(i) + 1u, cur)];
        float s = samplerTable[draw(ctx.key, tc, P_LIGHT + 3u * static_cast<uint32_t>(i) + 2u, cur)];
        if (r + s >= 1.0F) {
            r = 1.0F - r;
            s = 1.0F - s;
        }
        return l.triangle.pointA + r * l.triangle.AB + s * l.triangle.AC;
    }

    // direct lighting loop shared by both shaders (Whitted.cpp:37-64, PathTracer.cpp:48-79)
    void direct(Vec3* acc, const Intersection& it, Ctx ctx, uint32_t tc) {
        const int32_t rayDepth = it.ray.depth;
        for (int32_t i = 0; i < cfg.samplesLight; ++i) {
            const Light& light = lights[lightIndex(ctx, tc, i)];
            const Vec3 lightPos = lightPosition(light, ctx, tc, i);
            Vec3 vectorToLight = lightPos - it.point;
            const float distanceToLight = length(vectorToLight);
            vectorToLight = normalize(vectorToLight);
            const float cosNl = dot(it.normal, vectorToLight);
            if (cosNl > 0.0F) {
                Ray shadowRay(vectorToLight, it.point, rayDepth + 1, true, it.primitive, &rays);
                if (!shadowTrace(distanceToLight, shadowRay)) *acc += light.radiance.Le * cosNl;
            }
        }
    }

    bool shade(Vec3* rgb, const Intersection& it, Ctx ctx, uint32_t tc) {
        const int32_t rayDepth = it.ray.depth;
        if (cfg.shader == 3) {  // DepthMap.cpp:13-18
            const float maxDist = length(maxPoint - it.ray.origin) * 1.1F;
            const float depth = std::max((maxDist - it.length) / maxDist, 0.0F);
            *rgb = Vec3(depth, depth, depth);
            return false;
        }
        if (cfg.shader == 4) {  // DiffuseMaterial.cpp:12-28
            const Material& m = *it.material;
            if (hasPositiveValue(m.Kd)) {
                *rgb = m.Kd;
            } else if (hasPositiveValue(m.Ks)) {
                *rgb = m.Ks;
            } else if (hasPositiveValue(m.Kt)) {
                *rgb = m.Kt;
            } else if (hasPositiveValue(m.Le)) {
                *rgb = m.Le;
            }
            return false;
        }
        if (cfg.shader != 1 && cfg.shader != 2) {  // NoShadows.cpp:13-44 (C_wrapper.cpp:188-193 default)
            const Vec3& lE = it.material->Le;
            if (hasPositiveValue(lE)) {
                *rgb = lE;
                return true;
            }
            const Vec3& kD = it.material->Kd;
            if (hasPositiveValue(kD)) {
                if (!lights.empty()) {
                    for (int32_t j = 0; j < cfg.samplesLight; ++j) {
                        const Light& light = lights[lightIndex(ctx, tc, j)];
                        const Vec3 lightPos = lightPosition(light, ctx, tc, j);
                        const Vec3 toLight = normalize(lightPos - it.point);
                        const float cosNl = dot(it.normal, toLight);
                        if (cosNl > 0.0F) *rgb += light.radiance.Le * cosNl;
                    }
                    *rgb *= kD;
                    *rgb /= static_cast<float>(cfg.samplesLight);
                }
            }
            *rgb += kD * 0.1F;
            return false;
        }
        if (rayDepth > cfg.maxDepth) return false;
        const Vec3& lE = it.material->Le;
        if (hasPositiveValue(lE)) {
            *rgb = lE;
            return true;
        }
        const Vec3& kD = it.material->Kd;
        const Vec3& kS = it.material->Ks;
        const Vec3& kT = it.material->Kt;
        const Vec3& n = it.normal;
        if (cfg.shader == 1) {  // Whitted.cpp:13-93
            if (hasPositiveValue(kD) && !lights.empty()) {
                direct(rgb, it, ctx, tc);
                *rgb *= kD;
                *rgb /= static_cast<float>(cfg.samplesLight);
            }
            if (hasPositiveValue(kS)) {
                Ray specularRay(reflect(it.ray.direction, n), it.point, rayDepth + 1, false, it.primitive, &rays);
                Vec3 LiS_RGB;
                rayTrace(&LiS_RGB, specularRay, ctx, tc * 4u + 2u);
                *rgb += kS * LiS_RGB;
            }
            if (hasPositiveValue(kT)) {
                Ray transmissionRay(refract(it.ray.direction, n, 1.0F / it.material->ior), it.point, rayDepth + 1, false,
                                    it.primitive, &rays);
                Vec3 LiT_RGB;
                rayTrace(&LiT_RGB, transmissionRay, ctx, tc * 4u + 3u);
                *rgb += kT * LiT_RGB;
            }
            *rgb += kD * 0.1F;
            return false;
        }
        // PathTracer.cpp:22-142
        Vec3 Ld, LiD, LiS, LiT;
        bool intersectedLight = false;
        if (hasPositiveValue(kD)) {
            if (!lights.empty()) {
                direct(&Ld, it, ctx, tc);
                Ld *= kD;
                Ld /= static_cast<float>(cfg.samplesLight);
            }
            if (rayDepth <= RayDepthMin || samplerTable[draw(ctx.key, tc, P_RUSSIAN, curRR)] > 0.5F) {
                const Vec3 newDirection = cosineSampleHemisphere(n, ctx, tc);
                Ray secondary(newDirection, it.point, rayDepth + 1, false, it.primitive, &rays);
                Vec3 LiD_RGB;
                intersectedLight = rayTrace(&LiD_RGB, secondary, ctx, tc * 4u + 1u);
                LiD += kD * LiD_RGB;
                if (rayDepth > RayDepthMin) LiD /= 0.5F * 0.5F;
                if (hasPositiveValue(Ld) && intersectedLight) LiD = Vec3();
            }
        }
        if (hasPositiveValue(kS)) {
            Ray specularRay(reflect(it.ray.direction, n), it.point, rayDepth + 1, false, it.primitive, &rays);
            Vec3 LiS_RGB;
            rayTrace(&LiS_RGB, specularRay, ctx, tc * 4u + 2u);
            LiS += kS * LiS_RGB;
        }
        if (hasPositiveValue(kT)) {
            Ray transmissionRay(refract(it.ray.direction, n, 1.0F / it.material->ior), it.point, rayDepth + 1, false,
                                it.primitive, &rays);
            Vec3 LiT_RGB;
            rayTrace(&LiT_RGB, transmissionRay, ctx, tc * 4u + 3u);
            LiT += kT * LiT_RGB;
        }
        *rgb += Ld;
        *rgb += LiD;
        *rgb += LiS;
        *rgb += LiT;
        return intersectedLight;
    }

    // distinct reference tiles (Renderer.cpp:117-135): x0, y0 of each
    std::vector<std::array<int, 2>> tiles() const {
        const int W = cfg.width, H = cfg.height;
        const int bx = W / 16, by = H / 16;
        const int domainSize = (W / bx) * (H / by);
        std::vector<int> blocks;
        for (int j = 0; j < NumberOfTiles; ++j) {
            const float tile = static_cast<float>(j) / NumberOfTiles;
            const int rb = static_cast<int>(::roundf(tile * domainSize));
            if (std::find(blocks.begin(), blocks.end(), rb) == blocks.end()) blocks.push_back(rb);
        }
        std::vector<std::array<int, 2>> out;
        for (int rb : blocks) {
            const int pixel = rb * bx % (W * H);
            out.push_back({pixel % W, ((pixel / W) * by) % H});
        }
        return out;
    }

    Ray cameraRay(int x, int y, int sample, uint32_t* keyOut) {
        const int W = cfg.width, H = cfg.height;
        const float invImgWidth = 1.0F / W, invImgHeight = 1.0F / H;
        const float pixelWidth = 0.5F / W, pixelHeight = 0.5F / H;
        const uint32_t key = pathKey(static_cast<uint32_t>(y * W + x), static_cast<uint32_t>(sample));
        float r1 = pixelValue, r2 = pixelValue;  // Constant(0.5) unless spp > 1 (C_wrapper.cpp:144-148)
        if (cfg.samplesPixel > 1) {
            r1 = samplerTable[draw(key, 0u, P_JITTER_U, curPixel)];
            r2 = samplerTable[draw(key, 0u, P_JITTER_V, curPixel)];
        }
        const float u = x * invImgWidth, v = y * invImgHeight;
        const float deviationU = (r1 - 0.5F) * 2.0F * pixelWidth;
        const float deviationV = (r2 - 0.5F) * 2.0F * pixelHeight;
        *keyOut = key;
        return camera.generateRay(u, v, deviationU, deviationV, &rays);
    }

    // Renderer::renderScene (Renderer.cpp:107-170) over a list of tiles
    void renderTiles(int32_t* bitmap, int threads, const std::vector<int>& list) {
        const auto ts = tiles();
        const int W = cfg.width, H = cfg.height, bx = W / 16, by = H / 16;
        std::atomic<size_t> next{0};
        auto worker = [&]() {
            // per-thread materials: the reference shares them between render threads (a textured
            // hit writes Kd_ that another thread may read); single-threaded order is the contract
            std::vector<Material> mats = materials;
            while (true) {
                const size_t n = next.fetch_add(1);
                if (n >= list.size()) break;
                const int k = list[n];
                if (k < 0 || k >= static_cast<int>(ts.size())) continue;
                const int startX = ts[static_cast<size_t>(k)][0], startY = ts[static_cast<size_t>(k)][1];
                for (int sample = 0; sample < cfg.samplesPixel; ++sample) {
                    for (int y = startY; y < startY + by; ++y) {
                        for (int x = startX; x < startX + bx; ++x) {
                            const int64_t idx = static_cast<int64_t>(y) * W + x;
                            if (idx >= static_cast<int64_t>(W) * H) continue;
                            uint32_t key;
                            const Ray ray = cameraRay(x, y, sample, &key);
                            Vec3 pixelRgb;
                            rayTrace(&pixelRgb, ray, Ctx{key, &mats}, 1u);
                            bitmap[idx] = incrementalAvg(pixelRgb, bitmap[idx], sample + 1);
                        }
                    }
                }
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < threads; ++t) pool.emplace_back(worker);
        worker();
        for (auto& t : pool) t.join();
    }
};

Engine* create(const Config& cfg) {
    auto e = std::make_unique<Engine>();
    e->cfg = cfg;
    const float ratio = static_cast<float>(cfg.width) / cfg.height;
    Scene s;
    // C_wrapper.cpp:76-140; maxDist feeds DepthMap (shader 3)
    e->maxPoint = Vec3(1.0F, 1.0F, 1.0F);
    if (cfg.sceneIndex == 0) {
        cornellBox(&s, &e->camera, ratio);
    } else if (cfg.sceneIndex == 1) {
        spheres(&s, &e->camera, ratio);
        e->maxPoint = Vec3(8.0F, 8.0F, 8.0F);
    } else if (cfg.sceneIndex == 2) {
        cornellBox2(&s, &e->camera, ratio);
    } else if (cfg.sceneIndex == 3) {
        spheres2(&s, &e->camera, ratio);
        e->maxPoint = Vec3(8.0F, 8.0F, 8.0F);
    } else {
        std::string err;
        if (!loadObj(cfg.obj, cfg.mtl, &s, &err)) return nullptr;
        if (!loadCamera(cfg.cam, ratio, &e->camera)) return nullptr;
    }
    for (size_t i = 0; i < s.triangles.size(); ++i) s.triangles[i].inputIndex = static_cast<int64_t>(i);
    for (size_t i = 0; i < s.planes.size(); ++i) s.planes[i].inputIndex = static_cast<int64_t>(i);
    for (size_t i = 0; i < s.spheres.size(); ++i) s.spheres[i].inputIndex = static_cast<int64_t>(i);
    e->numTriangles = static_cast<int64_t>(s.triangles.size());
    e->materials = s.materials;
    e->lights = s.lights;
    e->planes = std::make_unique<BVH<Plane>>(s.planes);
    e->spheres = std::make_unique<BVH<Sphere>>(s.spheres);
    e->triangles = std::make_unique<BVH<Triangle>>(s.triangles);
    if (cfg.accelerator == 2) {
        e->gridPlanes = std::make_unique<RegularGrid<Plane>>(s.planes, 32U);
        e->gridSpheres = std::make_unique<RegularGrid<Sphere>>(s.spheres, 32U);
        e->gridTriangles = std::make_unique<RegularGrid<Triangle>>(s.triangles, 32U);
    }
    e->naivePlanes = s.planes;
    e->naiveSpheres = s.spheres;
    e->naiveTriangles = s.triangles;
    e->shaderTable = haltonTable(0x4D525400u);
    e->samplerTable = haltonTable(0x4D525401u);
    return e.release();
}

}  // namespace oracle

// ---- C API for the tests (ctypes) ---------------------------------------------------------
extern "C" {

struct OracleConfig {
    int32_t width, height, shader, sceneIndex, samplesPixel, samplesLight, maxDepth;
    const char* obj;
    const char* mtl;
    const char* cam;
    int32_t accelerator;
};

// a decoded texture for map_Kd lookups (path as the loader forms it: OBJ directory + name)
void oracle_register_texture(const char* path, int32_t width, int32_t height, int32_t channels, const uint8_t* data) {
    oracle::Texture t;
    t.width = width;
    t.height = height;
    t.channels = channels;
    t.image.assign(data, data + static_cast<size_t>(width) * static_cast<size_t>(height) * static_cast<size_t>(channels));
    oracle::textureRegistry()[path] = std::move(t);
}

void* oracle_create(const OracleConfig* c) {
    oracle::Config cfg{c->width, c->height, c->shader, c->sceneIndex, c->samplesPixel, c->samplesLight,
                       c->maxDepth > 0 ? c->maxDepth : 6, c->obj, c->mtl, c->cam, c->accelerator};
    return oracle::create(cfg);
}

void oracle_destroy(void* h) { delete static_cast<oracle::Engine*>(h); }

// a grid cell's membership test (Triangle.cpp:142-229, Plane.cpp:146-155, Sphere.cpp:102-123):
// kind 0 prim = A, B, C; 1 = point, normal; 2 = center, radius; box = min, max
int oracle_grid_box_test(int kind, const float* prim, const float* box) {
    using namespace oracle;
    const AABB b{Vec3(box[0], box[1], box[2]), Vec3(box[3], box[4], box[5])};
    const Vec3 p0(prim[0], prim[1], prim[2]), p1(prim[3], prim[4], prim[5]);
    if (kind == 0) return boxIntersect(Triangle::build(p0, p1, Vec3(prim[6], prim[7], prim[8]), nullptr, nullptr, nullptr, -1), b);
    if (kind == 1) return boxIntersect(Plane(p0, p1, -1), b);
    if (kind == 2) return boxIntersect(Sphere(p0, prim[3], -1), b);
    return -1;
}

// the RegularGrid of one kind (0 planes, 1 spheres, 2 triangles) of an accelerator-2 engine:
// world[12] = min, max, cellSize, cellSizeInverted; start[32^3 + 1]; items = input indices
int64_t oracle_regular_grid(void* h, int kind, float* world, int32_t* start, int32_t* items) {
    auto* e = static_cast<oracle::Engine*>(h);
    int64_t n = -1;
    auto dump = [&](const auto& g) {
        const oracle::Vec3 w[4] = {g->worldBoundaries.pointMin, g->worldBoundaries.pointMax, g->cellSize,
                                   g->cellSizeInverted};
        for (int i = 0; i < 4; ++i)
            for (int a = 0; a < 3; ++a)
                if (world != nullptr) world[3 * i + a] = w[i][a];
        int64_t k = 0;
        for (size_t c = 0; c < g->grid.size(); ++c) {
            if (start != nullptr) start[c] = static_cast<int32_t>(k);
            for (const auto* p : g->grid[c]) {
                if (items != nullptr) items[k] = static_cast<int32_t>(p->inputIndex);
                ++k;
            }
        }
        if (start != nullptr) start[g->grid.size()] = static_cast<int32_t>(k);
        n = k;
    };
    if (kind == 0 && e->gridPlanes) dump(e->gridPlanes);
    if (kind == 1 && e->gridSpheres) dump(e->gridSpheres);
    if (kind == 2 && e->gridTriangles) dump(e->gridTriangles);
    return n;
}

// timing-faithful sample draws (shared atomic cursors, as the reference): 1 on, 0 off
void oracle_set_faithful(void* h, int on) { static_cast<oracle::Engine*>(h)->faithful = on != 0; }
// the value of the Constant pixel sampler of 1 spp frames and camera rays (the reference's is 0.5)
void oracle_set_pixel_value(void* h, float value) { static_cast<oracle::Engine*>(h)->pixelValue = value; }

int oracle_num_tiles(void* h) { return static_cast<int>(static_cast<oracle::Engine*>(h)->tiles().size()); }

// Renderer::renderFrame over tiles [first, first + count); returns rays cast by this call
uint64_t oracle_render(void* h, int32_t* bitmap, int threads, int first, int count) {
    auto* e = static_cast<oracle::Engine*>(h);
    const uint64_t before = e->rays.load();
    std::vector<int> list;
    const int nt = static_cast<int>(e->tiles().size());
    for (int k = first; k < nt && k - first < count; ++k) list.push_back(k);
    e->renderTiles(bitmap, threads < 1 ? 1 : threads, list);
    return e->rays.load() - before;
}

// the same over an explicit tile list (bounded CPU-baseline samples)
uint64_t oracle_render_tiles(void* h, int32_t* bitmap, int threads, const int32_t* tiles, int n) {
    auto* e = static_cast<oracle::Engine*>(h);
    const uint64_t before = e->rays.load();
    e->renderTiles(bitmap, threads < 1 ? 1 : threads, std::vector<int>(tiles, tiles + n));
    return e->rays.load() - before;
}

void oracle_counts(void* h, int64_t* out) {
    auto* e = static_cast<oracle::Engine*>(h);
    out[0] = e->numTriangles;
    out[1] = static_cast<int64_t>(e->lights.size());
    out[2] = static_cast<int64_t>(e->planes->primitives.size());
    out[3] = static_cast<int64_t>(e->spheres->primitives.size());
    out[4] = static_cast<int64_t>(e->materials.size());
    out[5] = static_cast<int64_t>(e->triangles->boxes.size());
}

// camera-ray closest hit per pixel (sample 0); kind/index -1 for unrendered pixels
void oracle_primary_hits(void* h, int32_t* kind, int32_t* index, float* t) {
    auto* e = static_cast<oracle::Engine*>(h);
    const int W = e->cfg.width, H = e->cfg.height;
    for (int i = 0; i < W * H; ++i) {
        kind[i] = -1;
        index[i] = -1;
        t[i] = 0.0F;
    }
    const auto ts = e->tiles();
    const int bx = W / 16, by = H / 16;
    for (const auto& tile : ts) {
        for (int y = tile[1]; y < tile[1] + by; ++y) {
            for (int x = tile[0]; x < tile[0] + bx; ++x) {
                const int64_t idx = static_cast<int64_t>(y) * W + x;
                if (idx >= static_cast<int64_t>(W) * H) continue;
                uint32_t key;
                const oracle::Ray ray = e->cameraRay(x, y, 0, &key);
                oracle::Intersection it(ray);
                it = e->closest(it);
                const bool hit = it.length < oracle::RayLengthMax;
                kind[idx] = hit ? it.kind : 0;
                index[idx] = hit ? static_cast<int32_t>(it.index) : -1;
                t[idx] = it.length;
            }
        }
    }
}

// the primitive a (kind, input index) source pair names (Ray::primitive_), NULL where it names none
static const void* findSource(const oracle::Engine* e, int32_t k, int32_t j) {
    if (k == 3) {
        for (const auto& p : e->triangles->primitives) if (p.inputIndex == j) return &p;
    } else if (k == 1) {
        for (const auto& p : e->planes->primitives) if (p.inputIndex == j) return &p;
    } else if (k == 2) {
        for (const auto& p : e->spheres->primitives) if (p.inputIndex == j) return &p;
    } else if (k == 4) {
        for (const auto& l : e->lights) if (l.index == j) return &l.triangle;
    }
    return nullptr;
}

// Shader::rayTrace's intersection part (any = 0: kind / input index / t) or Shader::shadowTrace
// (any = 1, tmax dist[i]: kind[i] = occluded) of arbitrary rays; src: NULL or (kind, input
// index) pairs of the primitive each ray leaves (Ray::primitive_, self-exclusion)
void oracle_trace_rays(void* h, const float* o, const float* d, const float* dist, const int32_t* src, int32_t n,
                       int any, int32_t* kind, int32_t* index, float* t) {
    auto* e = static_cast<oracle::Engine*>(h);
    for (int32_t i = 0; i < n; ++i) {
        const oracle::Vec3 org(o[3 * i], o[3 * i + 1], o[3 * i + 2]);
        const oracle::Vec3 dir(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        const void* prim = src != nullptr ? findSource(e, src[2 * i], src[2 * i + 1]) : nullptr;
        if (any) {
            const oracle::Ray ray(dir, org, 2, true, prim, nullptr);
            kind[i] = e->shadowTrace(dist[i], ray) ? 1 : 0;
            index[i] = -1;
            t[i] = 0.0F;
        } else {
            const oracle::Ray ray(dir, org, 1, false, prim, nullptr);
            oracle::Intersection it(ray);
            it = e->closest(it);
            const bool hit = it.length < oracle::RayLengthMax;
            kind[i] = hit ? it.kind : 0;
            index[i] = hit ? static_cast<int32_t>(it.index) : -1;
            t[i] = it.length;
        }
    }
}

// Shader::rayTrace's `rgb` for arbitrary rays, before any conversion: ray i is the depth-1 ray of a
// path with key keys[i] (NULL: pathKey(i, 0)), src as for oracle_trace_rays.  With threads the rays
// are split statically, each worker on its own copy of the materials (as renderTiles' workers).
// Returns the rays cast by this call, the given ones included (a frame counts its camera rays).
uint64_t oracle_shade_rays(void* h, const float* o, const float* d, const uint32_t* keys, const int32_t* src, int32_t n,
                           int threads, float* rgb) {
    auto* e = static_cast<oracle::Engine*>(h);
    const uint64_t before = e->rays.load();
    const int nThreads = std::max(1, std::min(threads, n));
    auto worker = [&](int32_t first, int32_t last) {
        std::vector<oracle::Material> mats = e->materials;
        for (int32_t i = first; i < last; ++i) {
            const oracle::Vec3 org(o[3 * i], o[3 * i + 1], o[3 * i + 2]);
            const oracle::Vec3 dir(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
            const void* prim = src != nullptr ? findSource(e, src[2 * i], src[2 * i + 1]) : nullptr;
            const uint32_t key = keys != nullptr ? keys[i] : oracle::pathKey(static_cast<uint32_t>(i), 0u);
            const oracle::Ray ray(dir, org, 1, false, prim, &e->rays);
            oracle::Vec3 out;
            e->rayTrace(&out, ray, oracle::Engine::Ctx{key, &mats}, 1u);
            for (int a = 0; a < 3; ++a) rgb[3 * i + a] = out[a];
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nThreads; ++t)
        pool.emplace_back(worker, static_cast<int32_t>(static_cast<int64_t>(n) * t / nThreads),
                          static_cast<int32_t>(static_cast<int64_t>(n) * (t + 1) / nThreads));
    worker(0, static_cast<int32_t>(static_cast<int64_t>(n) / nThreads));
    for (auto& t : pool) t.join();
    return e->rays.load() - before;
}

// the frame's camera rays (Engine::cameraRay): tiles in order, the pixels of a tile row by row,
// samples sampleBase .. sampleBase + spp - 1 innermost; only pixels with idx < W * H.  Returns the
// count; with o == NULL nothing is written.
int64_t oracle_camera_rays(void* h, int sampleBase, int spp, float* o, float* d, uint32_t* keys, int32_t* pixels) {
    auto* e = static_cast<oracle::Engine*>(h);
    const int W = e->cfg.width, H = e->cfg.height, bx = W / 16, by = H / 16;
    int64_t n = 0;
    for (const auto& tile : e->tiles()) {
        for (int y = tile[1]; y < tile[1] + by; ++y) {
            for (int x = tile[0]; x < tile[0] + bx; ++x) {
                const int64_t idx = static_cast<int64_t>(y) * W + x;
                if (idx >= static_cast<int64_t>(W) * H) continue;
                for (int s = sampleBase; s < sampleBase + spp; ++s, ++n) {
                    if (o == nullptr) continue;
                    uint32_t key;
                    const oracle::Ray ray = e->cameraRay(x, y, s, &key);
                    for (int a = 0; a < 3; ++a) {
                        o[3 * n + a] = ray.origin[a];
                        d[3 * n + a] = ray.direction[a];
                    }
                    keys[n] = key;
                    pixels[n] = static_cast<int32_t>(idx);
                }
            }
        }
    }
    return n;
}

// reference-numbered BVH of the triangles: boxes (n x 6), indexOffset, numPrimitives, prim order
int64_t oracle_triangle_bvh(void* h, float* boxes, int32_t* offsets, int32_t* counts, int32_t* order) {
    auto* e = static_cast<oracle::Engine*>(h);
    const auto& b = e->triangles->boxes;
    if (boxes != nullptr) {
        for (size_t i = 0; i < b.size(); ++i) {
            for (int a = 0; a < 3; ++a) {
                boxes[6 * i + a] = b[i].box.pointMin[a];
                boxes[6 * i + 3 + a] = b[i].box.pointMax[a];
            }
            offsets[i] = b[i].indexOffset;
            counts[i] = b[i].numPrimitives;
        }
        for (size_t i = 0; i < e->triangles->primitives.size(); ++i)
            order[i] = static_cast<int32_t>(e->triangles->primitives[i].inputIndex);
    }
    return static_cast<int64_t>(b.size());
}

// ---- KAT helpers (app/Unit_Testing) ----
// returns 1 if the ray hits the triangle (Triangle::intersect with a fresh Intersection)
int oracle_kat_triangle(const float* a, const float* b, const float* c, const float* orig, const float* dir,
                        int fromSelf, float* tOut) {
    using namespace oracle;
    const Triangle tri = Triangle::build(Vec3(a[0], a[1], a[2]), Vec3(b[0], b[1], b[2]), Vec3(c[0], c[1], c[2]), nullptr,
                                         nullptr, nullptr, -1);
    Ray ray(Vec3(dir[0], dir[1], dir[2]), Vec3(orig[0], orig[1], orig[2]), 1, true, fromSelf ? &tri : nullptr, nullptr);
    Intersection it(ray);
    const float last = it.length;
    it = tri.intersect(it);
    *tOut = it.length;
    return it.length < last ? 1 : 0;
}

int oracle_kat_aabb(const float* mn, const float* mx, const float* orig, const float* dir) {
    using namespace oracle;
    const AABB box{Vec3(mn[0], mn[1], mn[2]), Vec3(mx[0], mx[1], mx[2])};
    const Ray ray(Vec3(dir[0], dir[1], dir[2]), Vec3(orig[0], orig[1], orig[2]), 1, false, nullptr, nullptr);
    return box.intersect(ray) ? 1 : 0;
}

void oracle_aabb_props(const float* mn, const float* mx, float* centroid, float* area) {
    using namespace oracle;
    const AABB box{Vec3(mn[0], mn[1], mn[2]), Vec3(mx[0], mx[1], mx[2])};
    const Vec3 c = box.centroid();
    for (int i = 0; i < 3; ++i) centroid[i] = c[i];
    *area = box.surfaceArea();
}

void oracle_triangle_aabb(const float* a, const float* b, const float* c, float* mn, float* mx) {
    using namespace oracle;
    const Triangle tri = Triangle::build(Vec3(a[0], a[1], a[2]), Vec3(b[0], b[1], b[2]), Vec3(c[0], c[1], c[2]), nullptr,
                                         nullptr, nullptr, -1);
    const AABB box = tri.getAABB();
    for (int i = 0; i < 3; ++i) {
        mn[i] = box.pointMin[i];
        mx[i] = box.pointMax[i];
    }
}

int oracle_kat_plane(const float* point, const float* normal, const float* orig, const float* dir, float* tOut) {
    using namespace oracle;
    const Plane p(Vec3(point[0], point[1], point[2]), Vec3(normal[0], normal[1], normal[2]), -1);
    Ray ray(Vec3(dir[0], dir[1], dir[2]), Vec3(orig[0], orig[1], orig[2]), 19, false, nullptr, nullptr);
    Intersection it(ray);
    const float last = it.length;
    it = p.intersect(it);
    *tOut = it.length;
    return it.length < last ? 1 : 0;
}

int oracle_kat_sphere(const float* center, float radius, const float* orig, const float* dir, float* tOut) {
    using namespace oracle;
    const Sphere sp(Vec3(center[0], center[1], center[2]), radius, -1);
    Ray ray(Vec3(dir[0], dir[1], dir[2]), Vec3(orig[0], orig[1], orig[2]), 1, false, nullptr, nullptr);
    Intersection it(ray);
    const float last = it.length;
    it = sp.intersect(it);
    *tOut = it.length;
    return it.length < last ? 1 : 0;
}

void oracle_plane_aabb(const float* point, const float* normal, float* mn, float* mx) {
    using namespace oracle;
    const Plane p(Vec3(point[0], point[1], point[2]), Vec3(normal[0], normal[1], normal[2]), -1);
    const AABB box = p.getAABB();
    for (int i = 0; i < 3; ++i) {
        mn[i] = box.pointMin[i];
        mx[i] = box.pointMax[i];
    }
}

// Ray ids: two consecutive constructions increment the counter by one (TestRay.cpp:54-63)
int oracle_kat_ray_ids(void) {
    std::atomic<uint64_t> counter{0};
    const oracle::Ray r1(oracle::Vec3(10, 0, 10), oracle::Vec3(0, 0, 10), 19, false, nullptr, &counter);
    const uint64_t id1 = counter.load() - 1;
    const oracle::Ray r2(oracle::Vec3(10, 0, 10), oracle::Vec3(0, 0, 10), 19, false, nullptr, &counter);
    const uint64_t id2 = counter.load() - 1;
    (void)r1;
    (void)r2;
    return static_cast<int>(id2 - id1);
}

// camera file KAT (TestCameraLoader.cpp:19-49): pos, dir, up, hFov/vFov in degrees
int oracle_kat_camera(const char* path, float ratio, float* out) {
    oracle::Camera cam;
    if (!oracle::loadCamera(path, ratio, &cam)) return 0;
    for (int i = 0; i < 3; ++i) {
        out[i] = cam.position[i];
        out[3 + i] = cam.direction[i];
        out[6 + i] = cam.up[i];
        out[9 + i] = cam.right[i];
    }
    out[12] = (cam.hFov / oracle::kPi) * 180.0F;  // Camera.cpp:41-44 radToDeg
    out[13] = (cam.vFov / oracle::kPi) * 180.0F;
    return 1;
}

float oracle_halton(uint32_t index, uint32_t base) { return oracle::haltonSequence(index, base); }
// cos / sin of 2 pi r1 for every entry of the shader table (seed 0x4D525400), as the oracle's
// hemisphere sampler evaluates them: out[2i], out[2i + 1]
void oracle_hemisphere_trig(float* out) {
    const auto t = oracle::haltonTable(0x4D525400u);
    for (size_t i = 0; i < t.size(); ++i) oracle::hemisphereTrig(t[i], out + 2 * i, out + 2 * i + 1);
}
void oracle_table(uint32_t seed, float* out) {
    const auto t = oracle::haltonTable(seed);
    std::memcpy(out, t.data(), t.size() * sizeof(float));
}
uint32_t oracle_path_key(uint32_t pixel, uint32_t sample) { return oracle::pathKey(pixel, sample); }
uint32_t oracle_sample_index(uint32_t key, uint32_t tc, uint32_t purpose) { return oracle::sampleIndex(key, tc, purpose); }
int32_t oracle_incremental_avg(float r, float g, float b, int32_t avg, int32_t n) {
    return oracle::incrementalAvg(oracle::Vec3(r, g, b), avg, n);
}
float oracle_fast_arctan(float v) { return oracle::Camera::fastArcTan(v); }

// restated libstdc++ partition == std::partition on `trials` random arrays; returns mismatches
int oracle_selftest_partition(uint32_t seed, int trials) {
    std::mt19937 gen(seed);
    int bad = 0;
    for (int t = 0; t < trials; ++t) {
        std::uniform_int_distribution<int> len(0, 200), val(0, 99);
        const int n = len(gen);
        const int pivot = val(gen);
        std::vector<std::pair<int, int>> a(static_cast<size_t>(n));
        for (int i = 0; i < n; ++i) a[static_cast<size_t>(i)] = {val(gen), i};
        auto b = a;
        auto pred = [pivot](const std::pair<int, int>& x) { return x.first < pivot; };
        const auto ia = std::partition(a.begin(), a.end(), pred);
        const auto ib = oracle::libstdcxxPartition(b.begin(), b.end(), pred);
        if (a != b || (ia - a.begin()) != (ib - b.begin())) ++bad;
    }
    return bad;
}

}  // extern "C"
