// glsl_shim.h -- the part of GLSL the reference's compute shader uses, as C++20, so that the
// shader's own text (rewritten by oracle/glsl_rewrite.py into oracle/_ref/shader) compiles with
// g++ and can be compared with oracle/vcrt_oracle.c. TEST INFRASTRUCTURE ONLY.
//
// Everything here is ours: vector types with the swizzles the shader uses as members, operators
// written component-wise and left to right, and the built-ins bound to the canonical definitions
// of DESIGN.md section 3. Nothing comes from oracle/vcrt_oracle.c. sin and tan live in
// ref_builtins.cpp, which is compiled without -fsingle-precision-constant (this header and the
// shader are compiled with it, so that the shader's `0.5` and `1.` are floats as in GLSL); so
// every literal below carries an f suffix or is an integer.
//
// Include inside no namespace; it opens namespace ref_glsl, into which the including file also
// puts the shader, so that these sqrt / sin / tan / pow hide the C library's.
#pragma once

#include <cstdint>

extern "C" float ref_builtin_sin(float x);  // vcrt::sin_canonical (csrc/vcrt_math.h, host path)
extern "C" float ref_builtin_tan(float x);  // (float)tan((double)x)

namespace ref_glsl {

struct vec2;
struct vec3;
struct ivec2;

// ---- swizzle members: views of the owner's components, converted on use ------------------
template <int N, int A, int B>
struct swz2 {
    float d[N];
    operator vec2() const;
};
template <int N>
struct swz_rgb {
    float d[N];
    operator vec3() const;
    swz_rgb& operator+=(const vec3& v);
    swz_rgb& operator/=(float s);
};
template <int N>
struct uswz_xy {
    uint32_t d[N];
};

struct vec2 {
    union {
        struct { float x, y; };
        swz2<2, 0, 1> xy;
    };
    vec2() : x(0.0f), y(0.0f) {}
    vec2(float a, float b) : x(a), y(b) {}
};

struct vec3 {
    union {
        struct { float x, y, z; };
        swz2<3, 0, 1> xy;
        swz2<3, 0, 2> xz;
        swz2<3, 1, 2> yz;
    };
    vec3() : x(0.0f), y(0.0f), z(0.0f) {}  // an unset vector is vec3(0) (canonical)
    explicit vec3(float s) : x(s), y(s), z(s) {}
    vec3(float a, float b, float c) : x(a), y(b), z(c) {}
};

struct vec4 {
    union {
        struct { float x, y, z, w; };
        swz_rgb<4> rgb;
    };
    vec4() : x(0.0f), y(0.0f), z(0.0f), w(0.0f) {}
    vec4(float a, float b, float c, float e) : x(a), y(b), z(c), w(e) {}
};

struct uvec3 {
    union {
        struct { uint32_t x, y, z; };
        uswz_xy<3> xy;
    };
    uvec3() : x(0), y(0), z(0) {}
    uvec3(uint32_t a, uint32_t b, uint32_t c) : x(a), y(b), z(c) {}
};

struct ivec2 {
    int x, y;
    ivec2() : x(0), y(0) {}
    ivec2(int a, int b) : x(a), y(b) {}
    template <int N>
    explicit ivec2(const uswz_xy<N>& u) : x(static_cast<int>(u.d[0])), y(static_cast<int>(u.d[1])) {}
};

template <int N, int A, int B>
inline swz2<N, A, B>::operator vec2() const { return vec2(d[A], d[B]); }

// ---- operators: component-wise, x then y then z ---------------------------------------------
inline vec3 operator+(const vec3& a, const vec3& b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline vec3 operator-(const vec3& a, const vec3& b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline vec3 operator*(const vec3& a, const vec3& b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline vec3 operator*(float s, const vec3& a) { return vec3(s * a.x, s * a.y, s * a.z); }
inline vec3 operator*(const vec3& a, float s) { return vec3(a.x * s, a.y * s, a.z * s); }
inline vec3 operator/(const vec3& a, float s) { return vec3(a.x / s, a.y / s, a.z / s); }
inline vec3 operator-(const vec3& a) { return vec3(-a.x, -a.y, -a.z); }
inline vec3& operator*=(vec3& a, const vec3& b) { a = a * b; return a; }

template <int N>
inline swz_rgb<N>::operator vec3() const { return vec3(d[0], d[1], d[2]); }
template <int N>
inline swz_rgb<N>& swz_rgb<N>::operator+=(const vec3& v) {
    d[0] = d[0] + v.x; d[1] = d[1] + v.y; d[2] = d[2] + v.z;
    return *this;
}
template <int N>
inline swz_rgb<N>& swz_rgb<N>::operator/=(float s) {
    d[0] = d[0] / s; d[1] = d[1] / s; d[2] = d[2] / s;
    return *this;
}

// ---- built-ins ("Canonical math") ----------------------------------------
inline float sqrt(float x) { return __builtin_sqrtf(x); }  // correctly rounded
inline float sin(float x) { return ref_builtin_sin(x); }
inline float tan(float x) { return ref_builtin_tan(x); }
inline float floor(float x) { return __builtin_floorf(x); }
inline float fract(float x) { return x - floor(x); }
inline float radians(float deg) { return deg * 0.017453292519943295f; }
// pow is canonical for the one exponent the shader uses: pow(x, 5) = ((x*x)*(x*x))*x for x >= 0,
// NaN below (GLSL leaves x < 0 undefined). Any other exponent stops the program.
inline float pow(float x, float y) {
    if (y != 5.0f) __builtin_trap();
    if (x < 0.0f) return __builtin_nanf("");
    return ((x * x) * (x * x)) * x;
}
inline float dot(const vec2& a, const vec2& b) { return a.x * b.x + a.y * b.y; }
inline float dot(const vec3& a, const vec3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline float length(const vec3& a) { return sqrt(dot(a, a)); }
inline vec3 normalize(const vec3& a) { return a / sqrt(dot(a, a)); }
inline vec3 cross(const vec3& a, const vec3& b) {  // GLSL: (x1*y2 - y1*x2, x2*y0 - y2*x0, ...)
    return vec3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y);
}
inline vec3 reflect(const vec3& i, const vec3& n) { return i - (2.0f * dot(n, i)) * n; }
inline vec3 mix(const vec3& x, const vec3& y, float a) { return x * (1.0f - a) + y * a; }

// ---- what the shader expects around it ---------------------------------------------------------
struct sphere;                 // the shader's own struct (structures.glsl)
static const sphere* world;    // run-time view of the scene; the driver points it somewhere
static int ref_world_n;
inline int ref_world_length() { return ref_world_n; }

static long long ref_undefined_count;  // ray_color's flow off its end, made the canonical vec3(0)
inline vec3 ref_undefined_return() {
    ++ref_undefined_count;
    return vec3(0.0f);
}

struct image2D {};
static image2D OutputImage;
static uvec3 gl_GlobalInvocationID;
static ivec2 ref_stored_coord;
static vec4 ref_stored_color;
inline void imageStore(image2D&, const ivec2& p, const vec4& c) {
    ref_stored_coord = p;
    ref_stored_color = c;
}

}  // namespace ref_glsl
