// Test-only: the device counterpart of tests/hostsim/prim_check.cpp.  The arithmetic headers compiled for gfx950 - the
// generated column chains of fe_asm_gfx950.inc, the limb-per-lane form of fe_wide.hpp - behind batch entry points that take
// host arrays of `count` cases, so that tests/test_gpu_prims.py can compare them with big integers.  Never linked into the product.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -I<csrc> prim_check.hip -o _build/libdevprim.so
// Every entry point uploads its cases, launches one kernel, reads the results back and returns 0, or non-zero on any HIP error.
// Lane entry points: one lane per case, 64-thread workgroups.  Wavefront entry points: one 64-lane workgroup per case.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "fe.hpp"
#include "sc.hpp"
#include "ge.hpp"
#include "fe_wide.hpp"

namespace {

// device buffers of one call: inputs are uploaded, outputs start as zeros and are read back by finish()
struct Job {
    struct Out { void* dev; void* host; size_t bytes; };
    std::vector<void*> bufs;
    std::vector<Out> outs;
    bool ok = true;
    ~Job() { for (void* p : bufs) (void)hipFree(p); }
    void* alloc(size_t bytes) {
        void* d = nullptr;
        if (!ok || hipMalloc(&d, bytes) != hipSuccess) { ok = false; return nullptr; }
        bufs.push_back(d);
        return d;
    }
    template <class T> const T* in(const T* host, size_t n) {
        void* d = alloc(n * sizeof(T));
        if (ok && hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) ok = false;
        return (const T*)d;
    }
    template <class T> T* out(T* host, size_t n) {
        void* d = alloc(n * sizeof(T));
        if (ok && hipMemset(d, 0, n * sizeof(T)) != hipSuccess) ok = false;
        if (ok) outs.push_back({d, host, n * sizeof(T)});
        return (T*)d;
    }
    int finish() {
        if (ok && hipGetLastError() != hipSuccess) ok = false;
        if (ok && hipDeviceSynchronize() != hipSuccess) ok = false;
        for (const Out& o : outs)
            if (ok && hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost) != hipSuccess) ok = false;
        return ok ? 0 : 1;
    }
};

template <class K> __global__ void __launch_bounds__(64) k_lane(K k, int count) {
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if (i < count) k(i);
}
template <class K> __global__ void __launch_bounds__(64) k_wave(K k) { k((int)blockIdx.x); }

template <class K> int run_lanes(Job& j, const K& k, int count) {
    if (j.ok) hipLaunchKernelGGL(k_lane<K>, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, 0, k, count);
    return j.finish();
}
template <class K> int run_waves(Job& j, const K& k, int count) {
    if (j.ok) hipLaunchKernelGGL(k_wave<K>, dim3((unsigned)count), dim3(64), 0, 0, k);
    return j.finish();
}

__device__ inline fe load_fe(const int32_t* l) { fe r; for (int i = 0; i < 9; i++) r.v[i] = l[i]; return r; }
__device__ inline void store_fe(const fe& a, int32_t* l) { for (int i = 0; i < 9; i++) l[i] = a.v[i]; }
__device__ inline void store_bytes(const uint8_t* s, uint8_t* d, int n) { for (int i = 0; i < n; i++) d[i] = s[i]; }
__device__ inline void load_bytes(const uint8_t* s, uint8_t* d, int n) { for (int i = 0; i < n; i++) d[i] = s[i]; }
__device__ inline void store_fe_bytes(const fe& a, uint8_t* d) { uint8_t t[32]; fe_tobytes(a, t); store_bytes(t, d, 32); }

// ---- field, one lane per case: raw signed limbs in, result limbs and the canonical bytes out
enum { OP_MUL, OP_MUL_F, OP_SQ, OP_CARRY, OP_INVERT, OP_POW22523 };
template <int OP> struct K_fe {
    const int32_t *a, *b;
    uint8_t* bytes;     // may be null
    int32_t* limbs;     // may be null
    __device__ void operator()(int i) const {
        const fe x = load_fe(a + 9 * i);
        fe r;
        if (OP == OP_MUL) r = fe_mul(x, load_fe(b + 9 * i));
        else if (OP == OP_MUL_F) r = fe_mul_f(x, load_fe(b + 9 * i));
        else if (OP == OP_SQ) r = fe_sq(x);
        else if (OP == OP_CARRY) r = fe_carry(x);
        else if (OP == OP_INVERT) r = fe_invert(x);
        else r = fe_pow22523(x);
        if (limbs) store_fe(r, limbs + 9 * i);
        if (bytes) store_fe_bytes(r, bytes + 32 * i);
    }
};
struct K_fe_canon {
    const int32_t* a;
    uint8_t* bytes;
    __device__ void operator()(int i) const { store_fe_bytes(load_fe(a + 9 * i), bytes + 32 * i); }
};
template <int OP> int fe_entry(const int32_t* a, const int32_t* b, int count, uint8_t* out_bytes, int32_t* out_limbs) {
    if (count <= 0) return count < 0;
    Job j;
    K_fe<OP> k;
    k.a = j.in(a, 9 * (size_t)count);
    k.b = b ? j.in(b, 9 * (size_t)count) : nullptr;
    k.bytes = out_bytes ? j.out(out_bytes, 32 * (size_t)count) : nullptr;
    k.limbs = out_limbs ? j.out(out_limbs, 9 * (size_t)count) : nullptr;
    return run_lanes(j, k, count);
}

// ---- table addition on raw limbs (hs_ge_madd_t_limbs' contract)
struct K_madd_t {
    const int32_t *p, *q, *neg;
    int32_t* limbs;
    uint8_t* bytes;
    __device__ void operator()(int i) const {
        ge a;
        a.X = load_fe(p + 36 * i); a.Y = load_fe(p + 36 * i + 9); a.Z = load_fe(p + 36 * i + 18); a.T = load_fe(p + 36 * i + 27);
        ge_niels n;
        n.yplusx = load_fe(q + 27 * i); n.yminusx = load_fe(q + 27 * i + 9); n.xy2d = load_fe(q + 27 * i + 18);
        const ge r = ge_madd_t(a, n, neg[i]);
        store_fe(r.X, limbs + 36 * i); store_fe(r.Y, limbs + 36 * i + 9); store_fe(r.Z, limbs + 36 * i + 18); store_fe(r.T, limbs + 36 * i + 27);
        store_fe_bytes(r.X, bytes + 128 * i); store_fe_bytes(r.Y, bytes + 128 * i + 32);
        store_fe_bytes(r.Z, bytes + 128 * i + 64); store_fe_bytes(r.T, bytes + 128 * i + 96);
    }
};

// ---- scalars: 32-byte little-endian strings (any 256-bit value) in, the canonical result out
enum { SC_MUL, SC_ADD, SC_SUB, SC_INV, SC_INV_VAR, SC_INV_FERMAT };
template <int OP> struct K_sc {
    const uint8_t *a, *b;
    uint8_t* out;
    __device__ void operator()(int i) const {
        uint8_t t[32], u[32];
        load_bytes(a + 32 * i, t, 32);
        const sc x = sc_mont_from_bytes_mod_order(t);
        sc r;
        if (OP == SC_MUL || OP == SC_ADD || OP == SC_SUB) {
            load_bytes(b + 32 * i, u, 32);
            const sc y = sc_mont_from_bytes_mod_order(u);
            r = OP == SC_MUL ? sc_mul(x, y) : OP == SC_ADD ? sc_add(x, y) : sc_sub(x, y);
        } else {
            r = OP == SC_INV ? sc_invert(x) : OP == SC_INV_VAR ? sc_invert_var(x) : sc_invert_fermat(x);
        }
        sc_mont_tobytes(r, t);
        store_bytes(t, out + 32 * i, 32);
    }
};
template <int OP> int sc_entry(const uint8_t* a, const uint8_t* b, int count, uint8_t* out) {
    if (count <= 0) return count < 0;
    Job j;
    K_sc<OP> k;
    k.a = j.in(a, 32 * (size_t)count);
    k.b = b ? j.in(b, 32 * (size_t)count) : nullptr;
    k.out = j.out(out, 32 * (size_t)count);
    return run_lanes(j, k, count);
}
struct K_sc_wide {
    const uint8_t* a;
    uint8_t* out;
    __device__ void operator()(int i) const {
        uint8_t w[64], t[32];
        load_bytes(a + 64 * i, w, 64);
        sc_mont_tobytes(sc_mont_from_wide(w), t);
        store_bytes(t, out + 32 * i, 32);
    }
};

// ---- group (the contracts of the hs_ functions of the same names)
struct K_decompress_recompress {
    const uint8_t* in;
    int32_t* ok;
    uint8_t* out;
    __device__ void operator()(int i) const {
        uint8_t s[32], t[32];
        load_bytes(in + 32 * i, s, 32);
        ge p;
        const int good = ge_decompress(s, p);
        ok[i] = good;
        if (good) {
            ge_compress(p, t);
            store_bytes(t, out + 32 * i, 32);
        }
    }
};
struct K_uniform {
    const uint8_t* in;
    uint8_t* out;
    __device__ void operator()(int i) const {
        uint8_t w[64], t[32];
        load_bytes(in + 64 * i, w, 64);
        ge_compress(ge_from_uniform_bytes(w), t);
        store_bytes(t, out + 32 * i, 32);
    }
};
// P+Q, P-Q, P+niels(Q), P-niels(Q) on compressed inputs
struct K_addsub {
    const uint8_t *a, *b;
    int32_t* ok;
    uint8_t* out;
    __device__ void operator()(int i) const {
        uint8_t s[32], t[32];
        ge p, q;
        load_bytes(a + 32 * i, s, 32);
        int good = ge_decompress(s, p);
        load_bytes(b + 32 * i, s, 32);
        good &= ge_decompress(s, q);
        ok[i] = good;
        if (!good) return;
        const ge_cached c = ge_to_cached(q);
        const ge_niels n = ge_to_niels(q);
        ge_compress(ge_add(p, c), t); store_bytes(t, out + 128 * i, 32);
        ge_compress(ge_sub(p, c), t); store_bytes(t, out + 128 * i + 32, 32);
        ge_compress(ge_madd(p, n, 0), t); store_bytes(t, out + 128 * i + 64, 32);
        ge_compress(ge_madd(p, n, 1), t); store_bytes(t, out + 128 * i + 96, 32);
    }
};
// k*B by double-and-add
struct K_basemul {
    const uint8_t* k;
    uint8_t* out;
    __device__ void operator()(int i) const {
        uint8_t s[32], t[32];
        load_bytes(k + 32 * i, s, 32);
        ge acc = ge_identity(), base = ge_basepoint();
#pragma unroll 1
        for (int bit = 0; bit < 256; bit++) {
            if ((s[bit >> 3] >> (bit & 7)) & 1) acc = ge_add_ge(acc, base);
            base = ge_dbl(base);
        }
        ge_compress(acc, t);
        store_bytes(t, out + 32 * i, 32);
    }
};

// ---- wavefront form (fe_wide.hpp): one 64-lane workgroup per case
struct K_fw_mul {
    const int32_t *a, *b;
    int32_t* out;   // 19 words per case: the result word of lanes 0..18
    __device__ void operator()(int i) const {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t lane = threadIdx.x & 63u;
        const int32_t A = lane < 9u ? a[9 * i + lane] : 0, B = lane < 9u ? b[9 * i + lane] : 0;
        const int32_t r = fw_mul(A, B, fw_make_masks());
        if (lane < 19u) out[19 * i + lane] = r;
#endif
    }
};
struct K_pow22523_wave {
    const int32_t* a;
    uint8_t* bytes;
    int32_t* limbs;
    __device__ void operator()(int i) const {
#if defined(__HIP_DEVICE_COMPILE__)
        const fe r = fe_pow22523_wave(load_fe(a + 9 * i));   // the element is uniform across the wavefront
        if ((threadIdx.x & 63u) == 0) {
            store_fe(r, limbs + 9 * i);
            store_fe_bytes(r, bytes + 32 * i);
        }
#endif
    }
};

}  // namespace

extern "C" {
int dp_fe_mul_limbs(const int32_t* a, const int32_t* b, int count, uint8_t* out_bytes, int32_t* out_limbs) { return fe_entry<OP_MUL>(a, b, count, out_bytes, out_limbs); }
int dp_fe_mul_f_limbs(const int32_t* a, const int32_t* b, int count, uint8_t* out_bytes, int32_t* out_limbs) { return fe_entry<OP_MUL_F>(a, b, count, out_bytes, out_limbs); }
int dp_fe_sq_limbs(const int32_t* a, int count, uint8_t* out_bytes, int32_t* out_limbs) { return fe_entry<OP_SQ>(a, nullptr, count, out_bytes, out_limbs); }
int dp_fe_carry_limbs(const int32_t* a, int count, int32_t* out_limbs) { return fe_entry<OP_CARRY>(a, nullptr, count, nullptr, out_limbs); }
int dp_fe_invert(const int32_t* a, int count, uint8_t* out_bytes, int32_t* out_limbs) { return fe_entry<OP_INVERT>(a, nullptr, count, out_bytes, out_limbs); }
int dp_fe_pow22523(const int32_t* a, int count, uint8_t* out_bytes, int32_t* out_limbs) { return fe_entry<OP_POW22523>(a, nullptr, count, out_bytes, out_limbs); }
int dp_fe_canon_limbs(const int32_t* a, int count, uint8_t* out_bytes) {
    if (count <= 0) return count < 0;
    Job j;
    K_fe_canon k;
    k.a = j.in(a, 9 * (size_t)count);
    k.bytes = j.out(out_bytes, 32 * (size_t)count);
    return run_lanes(j, k, count);
}
// p: X Y Z T (4 x 9 limbs), q: y+x, y-x, 2dxy (3 x 9 limbs), negate: one flag per case; out: 4 x 9 limbs + the 4 canonical coordinates
int dp_ge_madd_t_limbs(const int32_t* p, const int32_t* q, const int32_t* negate, int count, int32_t* out_limbs, uint8_t* out_bytes) {
    if (count <= 0) return count < 0;
    Job j;
    K_madd_t k;
    k.p = j.in(p, 36 * (size_t)count);
    k.q = j.in(q, 27 * (size_t)count);
    k.neg = j.in(negate, (size_t)count);
    k.limbs = j.out(out_limbs, 36 * (size_t)count);
    k.bytes = j.out(out_bytes, 128 * (size_t)count);
    return run_lanes(j, k, count);
}
int dp_sc_mul(const uint8_t* a, const uint8_t* b, int count, uint8_t* out) { return sc_entry<SC_MUL>(a, b, count, out); }
int dp_sc_add(const uint8_t* a, const uint8_t* b, int count, uint8_t* out) { return sc_entry<SC_ADD>(a, b, count, out); }
int dp_sc_sub(const uint8_t* a, const uint8_t* b, int count, uint8_t* out) { return sc_entry<SC_SUB>(a, b, count, out); }
int dp_sc_inv(const uint8_t* a, int count, uint8_t* out) { return sc_entry<SC_INV>(a, nullptr, count, out); }
int dp_sc_inv_var(const uint8_t* a, int count, uint8_t* out) { return sc_entry<SC_INV_VAR>(a, nullptr, count, out); }
int dp_sc_inv_fermat(const uint8_t* a, int count, uint8_t* out) { return sc_entry<SC_INV_FERMAT>(a, nullptr, count, out); }
int dp_sc_wide(const uint8_t* a64, int count, uint8_t* out) {
    if (count <= 0) return count < 0;
    Job j;
    K_sc_wide k;
    k.a = j.in(a64, 64 * (size_t)count);
    k.out = j.out(out, 32 * (size_t)count);
    return run_lanes(j, k, count);
}
// ok[i] = ge_decompress accepted case i; out: its recompression (zeros where rejected)
int dp_decompress_recompress(const uint8_t* in, int count, int32_t* ok, uint8_t* out) {
    if (count <= 0) return count < 0;
    Job j;
    K_decompress_recompress k;
    k.in = j.in(in, 32 * (size_t)count);
    k.ok = j.out(ok, (size_t)count);
    k.out = j.out(out, 32 * (size_t)count);
    return run_lanes(j, k, count);
}
int dp_uniform(const uint8_t* in64, int count, uint8_t* out) {
    if (count <= 0) return count < 0;
    Job j;
    K_uniform k;
    k.in = j.in(in64, 64 * (size_t)count);
    k.out = j.out(out, 32 * (size_t)count);
    return run_lanes(j, k, count);
}
int dp_addsub(const uint8_t* a, const uint8_t* b, int count, int32_t* ok, uint8_t* out128) {
    if (count <= 0) return count < 0;
    Job j;
    K_addsub k;
    k.a = j.in(a, 32 * (size_t)count);
    k.b = j.in(b, 32 * (size_t)count);
    k.ok = j.out(ok, (size_t)count);
    k.out = j.out(out128, 128 * (size_t)count);
    return run_lanes(j, k, count);
}
int dp_basemul(const uint8_t* k32, int count, uint8_t* out) {
    if (count <= 0) return count < 0;
    Job j;
    K_basemul k;
    k.k = j.in(k32, 32 * (size_t)count);
    k.out = j.out(out, 32 * (size_t)count);
    return run_lanes(j, k, count);
}
// A and B limbs on lanes 0..8; out: the result word of lanes 0..18 (19 words per case)
int dp_fw_mul_limbs(const int32_t* a, const int32_t* b, int count, int32_t* out19) {
    if (count <= 0) return count < 0;
    Job j;
    K_fw_mul k;
    k.a = j.in(a, 9 * (size_t)count);
    k.b = j.in(b, 9 * (size_t)count);
    k.out = j.out(out19, 19 * (size_t)count);
    return run_waves(j, k, count);
}
int dp_fe_pow22523_wave(const int32_t* a, int count, uint8_t* out_bytes, int32_t* out_limbs) {
    if (count <= 0) return count < 0;
    Job j;
    K_pow22523_wave k;
    k.a = j.in(a, 9 * (size_t)count);
    k.bytes = j.out(out_bytes, 32 * (size_t)count);
    k.limbs = j.out(out_limbs, 9 * (size_t)count);
    return run_waves(j, k, count);
}
}
