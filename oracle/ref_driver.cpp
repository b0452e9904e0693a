// ref_driver: runs the reference's own classes on inputs read from a file and writes what they return
// to a file, for tests/golden/make_reference_fixtures.py.  Built by oracle/ref_build.py against the
// reference tree (its headers are included by path) and the stand-in headers of oracle/refshim/.
//
// Files are sequences of records: an int32 count of 4-byte words, then the words (float32 / int32,
// little-endian).  Modes:
//   frame  <scene> <shader> <accelerator> <width> <height> <out>
//          out: bitmap (w * h), casted rays (low word, high word)
//   mesh   <in> <out> <width> <height>
//          in : triangle points A B C (T x 9), triangle material (T), materials (M x 13: Le Kd Ks Kt ior),
//               light kind (L), light points A B C (L x 9), light materials (L x 13),
//               camera (12: kind, position, lookAt, up, a, b), DepthMap bound (3),
//               ray origins (N x 3), directions (N x 3), occlusion distances (N)
//          out: per accelerator 1, 2, 3: hit kind, input index, t bits, occluded (N each), the DepthMap
//               frame, its casted rays (2), the DiffuseMaterial frame, its casted rays (2);
//               then the BVH's reordered primitive list and the RegularGrid's primitive list (T each)
//   camera <in> <out>
//          in : cameras (C x 12; kind 0 Perspective, 1 Orthographic, 10-13 the built-in camera of scene
//               kind - 10 with ratio a), rows (R x 4: u, v, deviationU, deviationV)
//          out: per camera: origins (R x 3), directions (R x 3)
//   kat    <in> <out>
//          in : triangle cases (n x 15: A B C origin direction), plane cases (n x 12: point normal origin
//               direction), sphere cases (n x 10: centre radius origin direction), box cases (n x 12: min max
//               origin direction)
//          out: triangle hit, t; plane hit, t; sphere hit, t; box hit
//   avg    <in> <out>
//          in : rgb (n x 3), previous average (n), sample number (n);  out: incrementalAvg (n)
#include "Components/Cameras/Orthographic.hpp"
#include "Components/Cameras/Perspective.hpp"
#include "Components/Lights/AreaLight.hpp"
#include "Components/Lights/PointLight.hpp"
#include "Components/Samplers/Constant.hpp"
#include "Components/Shaders/DepthMap.hpp"
#include "Components/Shaders/DiffuseMaterial.hpp"
#include "Components/Shaders/NoShadows.hpp"
#include "Components/Shaders/Whitted.hpp"
#include "MobileRT/Accelerators/BVH.hpp"
#include "MobileRT/Accelerators/Naive.hpp"
#include "MobileRT/Accelerators/RegularGrid.hpp"
#include "MobileRT/Renderer.hpp"
#include "MobileRT/Scene.hpp"
#include "Scenes/Scenes.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {
using ::glm::vec3;
using ::MobileRT::Intersection;
using ::MobileRT::Material;
using ::MobileRT::Ray;
using ::MobileRT::Scene;
using ::MobileRT::Shader;
using ::MobileRT::Triangle;
using Words = std::vector<uint32_t>;

[[noreturn]] void die(const std::string& what) {
    std::fprintf(stderr, "ref_driver: %s\n", what.c_str());
    std::exit(2);
}

std::vector<Words> readRecords(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (f == nullptr) die(std::string("cannot read ") + path);
    std::vector<Words> out;
    int32_t n = 0;
    while (std::fread(&n, 4, 1, f) == 1) {
        if (n < 0) die("negative record length");
        Words w(static_cast<size_t>(n));
        if (n > 0 && std::fread(w.data(), 4, w.size(), f) != w.size()) die("short record");
        out.push_back(std::move(w));
    }
    std::fclose(f);
    return out;
}

struct Writer {
    std::FILE* f;
    explicit Writer(const char* path) : f(std::fopen(path, "wb")) {
        if (f == nullptr) die(std::string("cannot write ") + path);
    }
    ~Writer() { std::fclose(f); }
    void put(const void* data, size_t words) {
        const int32_t n = static_cast<int32_t>(words);
        std::fwrite(&n, 4, 1, f);
        if (words > 0) std::fwrite(data, 4, words, f);
    }
    void put(const std::vector<int32_t>& v) { put(v.data(), v.size()); }
    void put(const std::vector<float>& v) { put(v.data(), v.size()); }
    void putCount(uint64_t c) {
        const uint32_t w[2] = {static_cast<uint32_t>(c), static_cast<uint32_t>(c >> 32)};
        put(w, 2);
    }
};

float asFloat(uint32_t w) {
    float x;
    std::memcpy(&x, &w, 4);
    return x;
}
int32_t asInt(uint32_t w) { return static_cast<int32_t>(w); }
vec3 vec3At(const Words& w, size_t i) { return vec3{asFloat(w[i]), asFloat(w[i + 1]), asFloat(w[i + 2])}; }
void push3(std::vector<float>* out, const vec3& v) {
    for (int a = 0; a < 3; ++a) out->push_back(v[a]);
}

// Material(kD, kS, kT, ior, lE) from 13 floats Le Kd Ks Kt ior
Material materialAt(const Words& w, size_t i) {
    return Material{vec3At(w, i + 3), vec3At(w, i + 6), vec3At(w, i + 9), asFloat(w[i + 12]), vec3At(w, i)};
}

std::unique_ptr<::MobileRT::Camera> makeCamera(const Words& w, size_t i) {
    const int kind = static_cast<int>(asFloat(w[i]));
    const float a = asFloat(w[i + 10]), b = asFloat(w[i + 11]);
    switch (kind) {
        case 0: return std::make_unique<::Components::Perspective>(vec3At(w, i + 1), vec3At(w, i + 4), vec3At(w, i + 7), a, b);
        case 1: return std::make_unique<::Components::Orthographic>(vec3At(w, i + 1), vec3At(w, i + 4), vec3At(w, i + 7), a, b);
        case 10: return cornellBox_Cam(a);
        case 11: return spheres_Cam(a);
        case 12: return cornellBox_Cam(a);  // the reference pairs scene 2 with cornellBox_Cam
        case 13: return spheres2_Cam(a);
        default: die("unknown camera kind");
    }
}

std::unique_ptr<Shader> makeShader(int shader, Scene scene, const vec3& bound, int accelerator) {
    const auto acc = Shader::Accelerator(accelerator);
    switch (shader) {
        case 0: return std::make_unique<::Components::NoShadows>(std::move(scene), 1, acc);
        case 1: return std::make_unique<::Components::Whitted>(std::move(scene), 1, acc);
        case 3: return std::make_unique<::Components::DepthMap>(std::move(scene), bound, acc);
        case 4: return std::make_unique<::Components::DiffuseMaterial>(std::move(scene), acc);
        default: die("shader not supported here");
    }
}

// one frame at 1 spp with Constant(0.5) on one thread: the bitmap and the casted rays
uint64_t renderFrame(std::unique_ptr<Shader> shader, std::unique_ptr<::MobileRT::Camera> camera, int w, int h,
                     std::vector<int32_t>* bitmap) {
    bitmap->assign(static_cast<size_t>(w) * h, 0);
    ::MobileRT::Renderer renderer{std::move(shader), std::move(camera), std::make_unique<::Components::Constant>(0.5F),
                                  w, h, 1};
    renderer.renderFrame(bitmap->data(), 1);
    return renderer.getTotalCastedRays();
}

int modeFrame(char** a) {
    const int sceneIndex = std::atoi(a[0]), shader = std::atoi(a[1]), acc = std::atoi(a[2]);
    const int w = std::atoi(a[3]), h = std::atoi(a[4]);
    const float ratio = static_cast<float>(w) / h;
    Scene scene{};
    std::unique_ptr<::MobileRT::Camera> camera;
    vec3 bound{};
    switch (sceneIndex) {
        case 0: scene = cornellBox_Scene(std::move(scene)); camera = cornellBox_Cam(ratio); bound = vec3{1, 1, 1}; break;
        case 1: scene = spheres_Scene(std::move(scene)); camera = spheres_Cam(ratio); bound = vec3{8, 8, 8}; break;
        case 2: scene = cornellBox2_Scene(std::move(scene)); camera = cornellBox_Cam(ratio); bound = vec3{1, 1, 1}; break;
        case 3: scene = spheres2_Scene(std::move(scene)); camera = spheres2_Cam(ratio); bound = vec3{8, 8, 8}; break;
        default: die("built-in scenes are 0-3");
    }
    std::vector<int32_t> bitmap;
    const uint64_t rays = renderFrame(makeShader(shader, std::move(scene), bound, acc), std::move(camera), w, h, &bitmap);
    Writer out(a[5]);
    out.put(bitmap);
    out.putCount(rays);
    return 0;
}

struct Mesh {
    const Words &points, &material, &materials, &lightKind, &lightPoints, &lightMaterials;
    size_t numTriangles() const { return material.size(); }
    size_t numLights() const { return lightKind.size(); }
    // identity: every triangle's material index is its input index (the builds never read it)
    std::vector<Triangle> triangles(bool identity) const {
        std::vector<Triangle> out;
        out.reserve(numTriangles());
        for (size_t t = 0; t < numTriangles(); ++t) {
            out.emplace_back(Triangle::Builder(vec3At(points, 9 * t), vec3At(points, 9 * t + 3), vec3At(points, 9 * t + 6))
                                 .withMaterialIndex(identity ? static_cast<int32_t>(t) : asInt(material[t]))
                                 .build());
        }
        return out;
    }
    std::vector<std::unique_ptr<::MobileRT::Light>> lights() const {
        std::vector<std::unique_ptr<::MobileRT::Light>> out;
        for (size_t l = 0; l < numLights(); ++l) {
            const Material radiance = materialAt(lightMaterials, 13 * l);
            if (asInt(lightKind[l]) == 0) {
                out.emplace_back(std::make_unique<::Components::PointLight>(radiance, vec3At(lightPoints, 9 * l)));
            } else {
                out.emplace_back(std::make_unique<::Components::AreaLight>(
                    radiance, std::make_unique<::Components::Constant>(0.5F),
                    Triangle::Builder(vec3At(lightPoints, 9 * l), vec3At(lightPoints, 9 * l + 3), vec3At(lightPoints, 9 * l + 6))
                        .build()));
            }
        }
        return out;
    }
    Scene scene() const {
        Scene s{};
        s.triangles_ = triangles(false);
        for (size_t m = 0; m * 13 < materials.size(); ++m) s.materials_.emplace_back(materialAt(materials, 13 * m));
        s.lights_ = lights();
        return s;
    }
};

// Shader::rayTrace's intersection part and Shader::shadowTrace on a triangle accelerator and the lights
template <typename Accel>
void traceBatch(Accel* accel, const std::vector<std::unique_ptr<::MobileRT::Light>>& lights, const Words& orig,
                const Words& dirs, const Words& dist, Writer* out) {
    const size_t n = dist.size();
    std::vector<int32_t> kind(n), index(n), occluded(n);
    std::vector<float> t(n);
    for (size_t i = 0; i < n; ++i) {
        Intersection hit{Ray{vec3At(dirs, 3 * i), vec3At(orig, 3 * i), 1, false}};
        const float last = hit.length_;
        hit = accel->trace(hit);
        int32_t light = -1;
        for (size_t l = 0; l < lights.size(); ++l) {
            const float before = hit.length_;
            hit = lights[l]->intersect(std::move(hit));
            if (hit.length_ < before) light = static_cast<int32_t>(l);
        }
        const bool found = hit.length_ < last;
        kind[i] = !found ? 0 : (light >= 0 ? 4 : 3);
        index[i] = !found ? -1 : (light >= 0 ? light : hit.materialIndex_);
        t[i] = hit.length_;
        const float d = asFloat(dist[i]);
        Intersection shadow{Ray{vec3At(dirs, 3 * i), vec3At(orig, 3 * i), 2, true}, d};
        shadow = accel->shadowTrace(shadow);
        occluded[i] = shadow.length_ < d ? 1 : 0;
    }
    out->put(kind);
    out->put(index);
    out->put(t);
    out->put(occluded);
}

int modeMesh(char** a) {
    const std::vector<Words> in = readRecords(a[0]);
    if (in.size() != 11) die("mesh: 11 input records expected");
    const int w = std::atoi(a[2]), h = std::atoi(a[3]);
    const Mesh mesh{in[0], in[1], in[2], in[3], in[4], in[5]};
    const Words &camera = in[6], &bound = in[7], &orig = in[8], &dirs = in[9], &dist = in[10];
    if (in[0].size() != 9 * mesh.numTriangles() || camera.size() != 12 || bound.size() != 3 ||
        orig.size() != 3 * dist.size() || dirs.size() != 3 * dist.size())
        die("mesh: record sizes");
    Writer out(a[1]);
    const auto lights = mesh.lights();
    std::vector<int32_t> bvhOrder, gridOrder, bitmap;
    for (int acc = 1; acc <= 3; ++acc) {
        if (acc == 1) {
            ::MobileRT::Naive<Triangle> accel{mesh.triangles(true)};
            traceBatch(&accel, lights, orig, dirs, dist, &out);
        } else if (acc == 2) {
            ::MobileRT::RegularGrid<Triangle> accel{mesh.triangles(true), 32U};
            traceBatch(&accel, lights, orig, dirs, dist, &out);
            for (const Triangle& t : accel.getPrimitives()) gridOrder.push_back(t.getMaterialIndex());
        } else {
            ::MobileRT::BVH<Triangle> accel{mesh.triangles(true)};
            traceBatch(&accel, lights, orig, dirs, dist, &out);
            for (const Triangle& t : accel.getPrimitives()) bvhOrder.push_back(t.getMaterialIndex());
        }
        for (const int shader : {3, 4}) {
            const uint64_t rays = renderFrame(makeShader(shader, mesh.scene(), vec3At(bound, 0), acc), makeCamera(camera, 0),
                                              w, h, &bitmap);
            out.put(bitmap);
            out.putCount(rays);
        }
    }
    out.put(bvhOrder);
    out.put(gridOrder);
    return 0;
}

int modeCamera(char** a) {
    const std::vector<Words> in = readRecords(a[0]);
    if (in.size() != 2 || in[0].size() % 12 != 0 || in[1].size() % 4 != 0) die("camera: cameras and rows expected");
    Writer out(a[1]);
    const Words& rows = in[1];
    for (size_t c = 0; c * 12 < in[0].size(); ++c) {
        const auto camera = makeCamera(in[0], 12 * c);
        std::vector<float> orig, dirs;
        for (size_t r = 0; r * 4 < rows.size(); ++r) {
            const Ray ray{camera->generateRay(asFloat(rows[4 * r]), asFloat(rows[4 * r + 1]), asFloat(rows[4 * r + 2]),
                                              asFloat(rows[4 * r + 3]))};
            push3(&orig, ray.origin_);
            push3(&dirs, ray.direction_);
        }
        out.put(orig);
        out.put(dirs);
    }
    return 0;
}

// primitive.intersect on a fresh Intersection of one ray: hit flag and the length it leaves
template <typename Primitive>
void katOne(const Primitive& primitive, const Words& w, size_t rayAt, std::vector<int32_t>* hit, std::vector<float>* t) {
    Intersection it{Ray{vec3At(w, rayAt + 3), vec3At(w, rayAt), 1, false}};
    const float last = it.length_;
    it = primitive.intersect(it);
    hit->push_back(it.length_ < last ? 1 : 0);
    t->push_back(it.length_);
}

int modeKat(char** a) {
    const std::vector<Words> in = readRecords(a[0]);
    if (in.size() != 4) die("kat: 4 input records expected");
    Writer out(a[1]);
    std::vector<int32_t> hit;
    std::vector<float> t;
    for (size_t i = 0; i + 15 <= in[0].size(); i += 15) {
        const Triangle tri{Triangle::Builder(vec3At(in[0], i), vec3At(in[0], i + 3), vec3At(in[0], i + 6)).build()};
        katOne(tri, in[0], i + 9, &hit, &t);
    }
    out.put(hit);
    out.put(t);
    hit.clear();
    t.clear();
    for (size_t i = 0; i + 12 <= in[1].size(); i += 12) {
        const ::MobileRT::Plane plane{vec3At(in[1], i), vec3At(in[1], i + 3), -1};
        katOne(plane, in[1], i + 6, &hit, &t);
    }
    out.put(hit);
    out.put(t);
    hit.clear();
    t.clear();
    for (size_t i = 0; i + 10 <= in[2].size(); i += 10) {
        const ::MobileRT::Sphere sphere{vec3At(in[2], i), asFloat(in[2][i + 3]), -1};
        katOne(sphere, in[2], i + 4, &hit, &t);
    }
    out.put(hit);
    out.put(t);
    hit.clear();
    for (size_t i = 0; i + 12 <= in[3].size(); i += 12) {
        const ::MobileRT::AABB box{vec3At(in[3], i), vec3At(in[3], i + 3)};
        const Ray ray{vec3At(in[3], i + 9), vec3At(in[3], i + 6), 1, false};
        hit.push_back(box.intersect(ray) ? 1 : 0);
    }
    out.put(hit);
    return 0;
}

int modeAvg(char** a) {
    const std::vector<Words> in = readRecords(a[0]);
    if (in.size() != 3 || in[0].size() != 3 * in[1].size() || in[2].size() != in[1].size()) die("avg: rgb, average, n expected");
    std::vector<int32_t> res;
    for (size_t i = 0; i < in[1].size(); ++i)
        res.push_back(::MobileRT::incrementalAvg(vec3At(in[0], 3 * i), asInt(in[1][i]), asInt(in[2][i])));
    Writer out(a[1]);
    out.put(res);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "frame" && argc == 8) return modeFrame(argv + 2);
    if (mode == "mesh" && argc == 6) return modeMesh(argv + 2);
    if (mode == "camera" && argc == 4) return modeCamera(argv + 2);
    if (mode == "kat" && argc == 4) return modeKat(argv + 2);
    if (mode == "avg" && argc == 4) return modeAvg(argv + 2);
    std::fprintf(stderr, "usage: ref_driver frame|mesh|camera|kat|avg ... (see the head of ref_driver.cpp)\n");
    return 2;
}
