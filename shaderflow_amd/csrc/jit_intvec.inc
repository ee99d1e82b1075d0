// jit_intvec.inc — the three integer vector types of one scalar type (included by jit_runtime.hpp once for int, once for
// uint). Expects SF_RT_T (scalar), SF_RT_V2/3/4 (the types defined here), SF_RT_O2/3/4 (the other integer family).
// Same shape as the float vectors: a union of component names, an array and every GLSL swizzle.

struct bvec2; struct bvec3; struct bvec4;      // defined after both integer families (jit_runtime.hpp)

// T(v) is the first component (§5.4.1); ++ and -- add and subtract one at every component (§5.9)
#define SF_RT_INT_COMMON(V, N) \
    template <class S, typename std::enable_if<std::is_arithmetic<S>::value, int>::type = 0> \
    SF_HD explicit operator S() const { return (S)d[0]; } \
    SF_HD V& operator++() { for (int k = 0; k < N; k++) d[k] = d[k] + 1; return *this; } \
    SF_HD V& operator--() { for (int k = 0; k < N; k++) d[k] = d[k] - 1; return *this; } \
    SF_HD V operator++(int) { const V before = *this; ++*this; return before; } \
    SF_HD V operator--(int) { const V before = *this; --*this; return before; }

struct SF_RT_V2 {
    union {
        struct { SF_RT_T x, y; }; struct { SF_RT_T r, g; }; struct { SF_RT_T s, t; };
        SF_RT_T d[2];
#define SF_RT_A(n, ...) SwzT<SF_RT_T, SF_RT_V2, 2, __VA_ARGS__> n;
#define SF_RT_B(n, ...) SwzT<SF_RT_T, SF_RT_V3, 2, __VA_ARGS__> n;
#define SF_RT_C(n, ...) SwzT<SF_RT_T, SF_RT_V4, 2, __VA_ARGS__> n;
        SF_SWIZZLES_2(SF_RT_A, SF_RT_B, SF_RT_C)
#undef SF_RT_A
#undef SF_RT_B
#undef SF_RT_C
    };
    SF_HD SF_RT_V2() { x = 0; y = 0; }
    SF_HD explicit SF_RT_V2(SF_RT_T v) { x = v; y = v; }
    SF_HD SF_RT_V2(SF_RT_T a, SF_RT_T b) { x = a; y = b; }
    SF_HD explicit SF_RT_V2(const vec2& v);
    SF_HD explicit SF_RT_V2(const SF_RT_O2& v);
    SF_HD explicit SF_RT_V2(const bvec2& v);
    SF_HD SF_RT_V2(const SF_RT_V2& o) { for (int k = 0; k < 2; k++) d[k] = o.d[k]; }
    SF_HD SF_RT_V2& operator=(const SF_RT_V2& o) { for (int k = 0; k < 2; k++) d[k] = o.d[k]; return *this; }
    SF_HD SF_RT_T& operator[](int k) { return d[k]; }
    SF_HD SF_RT_T operator[](int k) const { return d[k]; }
    SF_RT_INT_COMMON(SF_RT_V2, 2)
};
struct SF_RT_V3 {
    union {
        struct { SF_RT_T x, y, z; }; struct { SF_RT_T r, g, b; }; struct { SF_RT_T s, t, p; };
        SF_RT_T d[3];
#define SF_RT_A(n, ...) SwzT<SF_RT_T, SF_RT_V2, 3, __VA_ARGS__> n;
#define SF_RT_B(n, ...) SwzT<SF_RT_T, SF_RT_V3, 3, __VA_ARGS__> n;
#define SF_RT_C(n, ...) SwzT<SF_RT_T, SF_RT_V4, 3, __VA_ARGS__> n;
        SF_SWIZZLES_3(SF_RT_A, SF_RT_B, SF_RT_C)
#undef SF_RT_A
#undef SF_RT_B
#undef SF_RT_C
    };
    SF_HD SF_RT_V3() { x = 0; y = 0; z = 0; }
    SF_HD explicit SF_RT_V3(SF_RT_T v) { x = v; y = v; z = v; }
    SF_HD SF_RT_V3(SF_RT_T a, SF_RT_T b, SF_RT_T c) { x = a; y = b; z = c; }
    SF_HD SF_RT_V3(const SF_RT_V2& a, SF_RT_T c) { x = a.x; y = a.y; z = c; }
    SF_HD SF_RT_V3(SF_RT_T a, const SF_RT_V2& b) { x = a; y = b.x; z = b.y; }
    SF_HD explicit SF_RT_V3(const vec3& v);
    SF_HD explicit SF_RT_V3(const SF_RT_O3& v);
    SF_HD explicit SF_RT_V3(const bvec3& v);
    SF_HD SF_RT_V3(const SF_RT_V3& o) { for (int k = 0; k < 3; k++) d[k] = o.d[k]; }
    SF_HD SF_RT_V3& operator=(const SF_RT_V3& o) { for (int k = 0; k < 3; k++) d[k] = o.d[k]; return *this; }
    SF_HD SF_RT_T& operator[](int k) { return d[k]; }
    SF_HD SF_RT_T operator[](int k) const { return d[k]; }
    SF_RT_INT_COMMON(SF_RT_V3, 3)
};
struct SF_RT_V4 {
    union {
        struct { SF_RT_T x, y, z, w; }; struct { SF_RT_T r, g, b, a; }; struct { SF_RT_T s, t, p, q; };
        SF_RT_T d[4];
#define SF_RT_A(n, ...) SwzT<SF_RT_T, SF_RT_V2, 4, __VA_ARGS__> n;
#define SF_RT_B(n, ...) SwzT<SF_RT_T, SF_RT_V3, 4, __VA_ARGS__> n;
#define SF_RT_C(n, ...) SwzT<SF_RT_T, SF_RT_V4, 4, __VA_ARGS__> n;
        SF_SWIZZLES_4(SF_RT_A, SF_RT_B, SF_RT_C)
#undef SF_RT_A
#undef SF_RT_B
#undef SF_RT_C
    };
    SF_HD SF_RT_V4() { x = 0; y = 0; z = 0; w = 0; }
    SF_HD explicit SF_RT_V4(SF_RT_T v) { x = v; y = v; z = v; w = v; }
    SF_HD SF_RT_V4(SF_RT_T a, SF_RT_T b, SF_RT_T c, SF_RT_T e) { x = a; y = b; z = c; w = e; }
    SF_HD SF_RT_V4(const SF_RT_V3& v, SF_RT_T e) { x = v.x; y = v.y; z = v.z; w = e; }
    SF_HD SF_RT_V4(const SF_RT_V2& u, const SF_RT_V2& v) { x = u.x; y = u.y; z = v.x; w = v.y; }
    SF_HD SF_RT_V4(const SF_RT_V2& u, SF_RT_T c, SF_RT_T e) { x = u.x; y = u.y; z = c; w = e; }
    SF_HD explicit SF_RT_V4(const vec4& v);
    SF_HD explicit SF_RT_V4(const SF_RT_O4& v);
    SF_HD explicit SF_RT_V4(const bvec4& v);
    SF_HD SF_RT_V4(const SF_RT_V4& o) { for (int k = 0; k < 4; k++) d[k] = o.d[k]; }
    SF_HD SF_RT_V4& operator=(const SF_RT_V4& o) { for (int k = 0; k < 4; k++) d[k] = o.d[k]; return *this; }
    SF_HD SF_RT_T& operator[](int k) { return d[k]; }
    SF_HD SF_RT_T operator[](int k) const { return d[k]; }
    SF_RT_INT_COMMON(SF_RT_V4, 4)
};
#undef SF_RT_INT_COMMON
