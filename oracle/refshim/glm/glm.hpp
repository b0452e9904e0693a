// Stand-in for the part of GLM that the reference's core uses (oracle/ref_build.py).  The arithmetic
// of every function is fixed by the project ("What is pinned to the reference itself"):
// plain float operations in the stated order, built without contraction.
#ifndef MRT_REFSHIM_GLM_HPP
#define MRT_REFSHIM_GLM_HPP
#include <cmath>
#include <sstream>
#include <string>
#include <type_traits>

namespace glm {
template <int L, typename T>
struct vec {
    T v[L];
    constexpr vec() : v{} {}
    template <typename S>
    constexpr explicit vec(S s) : v{} { for (int i = 0; i < L; ++i) v[i] = static_cast<T>(s); }
    template <typename A, typename B>
    constexpr vec(A a, B b) : v{static_cast<T>(a), static_cast<T>(b)} { static_assert(L == 2, "vec2 only"); }
    template <typename A, typename B, typename C>
    constexpr vec(A a, B b, C c) : v{static_cast<T>(a), static_cast<T>(b), static_cast<T>(c)} { static_assert(L == 3, "vec3 only"); }
    constexpr T& operator[](int i) { return v[i]; }
    constexpr const T& operator[](int i) const { return v[i]; }
    static constexpr int length() { return L; }
};
using vec2 = vec<2, float>;
using vec3 = vec<3, float>;

#define MRT_REFSHIM_OP(op) \
    template <int L, typename T> vec<L, T> operator op(const vec<L, T>& a, const vec<L, T>& b) { vec<L, T> r; for (int i = 0; i < L; ++i) r[i] = a[i] op b[i]; return r; } \
    template <int L, typename T> vec<L, T> operator op(const vec<L, T>& a, T s) { vec<L, T> r; for (int i = 0; i < L; ++i) r[i] = a[i] op s; return r; } \
    template <int L, typename T> vec<L, T> operator op(T s, const vec<L, T>& b) { vec<L, T> r; for (int i = 0; i < L; ++i) r[i] = s op b[i]; return r; } \
    template <int L, typename T> vec<L, T>& operator op##=(vec<L, T>& a, const vec<L, T>& b) { for (int i = 0; i < L; ++i) a[i] op##= b[i]; return a; } \
    template <int L, typename T, typename U, typename = typename std::enable_if<std::is_arithmetic<U>::value>::type> \
    vec<L, T>& operator op##=(vec<L, T>& a, U s) { for (int i = 0; i < L; ++i) a[i] op##= static_cast<T>(s); return a; }
MRT_REFSHIM_OP(+)
MRT_REFSHIM_OP(-)
MRT_REFSHIM_OP(*)
MRT_REFSHIM_OP(/)
#undef MRT_REFSHIM_OP
template <int L, typename T> vec<L, T> operator-(const vec<L, T>& a) { vec<L, T> r; for (int i = 0; i < L; ++i) r[i] = -a[i]; return r; }
template <int L, typename T> bool operator==(const vec<L, T>& a, const vec<L, T>& b) { for (int i = 0; i < L; ++i) if (!(a[i] == b[i])) return false; return true; }
template <int L, typename T> bool operator!=(const vec<L, T>& a, const vec<L, T>& b) { return !(a == b); }

template <typename T> T min(T a, T b) { return (b < a) ? b : a; }
template <typename T> T max(T a, T b) { return (a < b) ? b : a; }
template <int L, typename T> vec<L, T> min(const vec<L, T>& a, const vec<L, T>& b) { vec<L, T> r; for (int i = 0; i < L; ++i) r[i] = (b[i] < a[i]) ? b[i] : a[i]; return r; }
template <int L, typename T> vec<L, T> max(const vec<L, T>& a, const vec<L, T>& b) { vec<L, T> r; for (int i = 0; i < L; ++i) r[i] = (a[i] < b[i]) ? b[i] : a[i]; return r; }
template <typename T> T clamp(T x, T lo, T hi) { return min(max(x, lo), hi); }
inline float fract(float x) { return x - std::floor(x); }
template <int L, typename T> vec<L, T> fract(const vec<L, T>& a) { vec<L, T> r; for (int i = 0; i < L; ++i) r[i] = a[i] - std::floor(a[i]); return r; }

template <typename T> T dot(const vec<2, T>& a, const vec<2, T>& b) { const vec<2, T> p = a * b; return p[0] + p[1]; }
template <typename T> T dot(const vec<3, T>& a, const vec<3, T>& b) { const vec<3, T> p = a * b; return p[0] + p[1] + p[2]; }
template <typename T> vec<3, T> cross(const vec<3, T>& x, const vec<3, T>& y) {
    return vec<3, T>(x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]);
}
template <int L, typename T> T length(const vec<L, T>& a) { return std::sqrt(dot(a, a)); }
template <int L, typename T> vec<L, T> normalize(const vec<L, T>& a) { return a * (static_cast<T>(1) / std::sqrt(dot(a, a))); }
template <int L, typename T> vec<L, T> reflect(const vec<L, T>& I, const vec<L, T>& N) { return I - N * dot(N, I) * static_cast<T>(2); }
template <int L, typename T> vec<L, T> refract(const vec<L, T>& I, const vec<L, T>& N, T eta) {
    const T d = dot(N, I);
    const T k = static_cast<T>(1) - eta * eta * (static_cast<T>(1) - d * d);
    return (k >= static_cast<T>(0)) ? (eta * I - (eta * d + std::sqrt(k)) * N) : vec<L, T>(0);
}

template <int L, typename T> vec<L, bool> isnan(const vec<L, T>& a) { vec<L, bool> r; for (int i = 0; i < L; ++i) r[i] = std::isnan(a[i]); return r; }
template <int L, typename T> vec<L, bool> isinf(const vec<L, T>& a) { vec<L, bool> r; for (int i = 0; i < L; ++i) r[i] = std::isinf(a[i]); return r; }
template <int L, typename T> vec<L, bool> greaterThan(const vec<L, T>& a, const vec<L, T>& b) { vec<L, bool> r; for (int i = 0; i < L; ++i) r[i] = a[i] > b[i]; return r; }
template <int L> bool all(const vec<L, bool>& a) { for (int i = 0; i < L; ++i) if (!a[i]) return false; return true; }
template <int L> bool any(const vec<L, bool>& a) { for (int i = 0; i < L; ++i) if (a[i]) return true; return false; }

template <typename T> constexpr T pi() { return static_cast<T>(3.14159265358979323846264338327950288); }
template <typename T> constexpr T two_pi() { return static_cast<T>(6.28318530717958647692528676655900576); }
template <typename T> constexpr T quarter_pi() { return static_cast<T>(0.785398163397448309615660845819875721); }

template <int L, typename T> std::string to_string(const vec<L, T>& a) {
    std::ostringstream s;
    s << "vec" << L << "(";
    for (int i = 0; i < L; ++i) s << (i ? ", " : "") << a[i];
    s << ")";
    return s.str();
}
}  // namespace glm
#endif
