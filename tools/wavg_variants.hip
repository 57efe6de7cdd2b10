// wavg_variants.hip — experiment harness (not product code): variants of the wavg
// kernel and a compute-free streaming ceiling, timed interleaved in one process by
// tools/wavg_variants.py.  Same math as fhe-fed_amd/csrc/wavg.hip wavg_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct TC {
  uint64_t q, one_shoup, r30, r30_shoup, r60, r60_shoup;
};
struct Args {
  const uint64_t* ptrs[16];
  uint32_t wl[16][16][2];
  uint64_t* out;
  uint64_t rows;
  uint32_t C, L, logN, pad;
  TC tc[16];
};

__device__ __forceinline__ uint64_t addmod(uint64_t a, uint64_t b, uint64_t q) {
  uint64_t s = a + b;
  return s >= q ? s - q : s;
}
__device__ __forceinline__ uint64_t shoup_mul(uint64_t x, uint64_t w, uint64_t wp, uint64_t q) {
  uint64_t hi = __umul64hi(x, wp);
  uint64_t r = x * w - hi * q;
  return r >= q ? r - q : r;
}
__device__ __forceinline__ uint64_t red64(uint64_t x, uint64_t q, uint64_t one_sh) {
  uint64_t hi = __umul64hi(x, one_sh);
  uint64_t r = x - hi * q;
  return r >= q ? r - q : r;
}
__device__ __forceinline__ uint64_t fold(uint64_t s00, uint64_t s01, uint64_t s10, uint64_t s11,
                                         const TC& c) {
  uint64_t a = red64(s00, c.q, c.one_shoup);
  uint64_t m = red64(s01, c.q, c.one_shoup) + red64(s10, c.q, c.one_shoup);
  uint64_t b = shoup_mul(m, c.r30, c.r30_shoup, c.q);
  uint64_t d = shoup_mul(red64(s11, c.q, c.one_shoup), c.r60, c.r60_shoup, c.q);
  return addmod(addmod(a, b, c.q), d, c.q);
}

template <bool NT>
__device__ __forceinline__ u32x4 ld(const uint64_t* p) {
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return *reinterpret_cast<const u32x4*>(p);
}
template <bool NT>
__device__ __forceinline__ void st(uint64_t* p, u32x4 v) {
  if (NT) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
  else *reinterpret_cast<u32x4*>(p) = v;
}

// V = number of 16-byte vectors per thread per learner (2 residues each).
// PERSIST: grid-stride over chunks with a capped grid.
template <int V, bool NT, bool PERSIST, int THREADS>
__global__ __launch_bounds__(THREADS) void wavg_v(Args a, uint64_t nchunks) {
  constexpr uint32_t PER_BLOCK = 2 * V * THREADS;
  const uint32_t M30 = (1u << 30) - 1;
  for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += (PERSIST ? gridDim.x : nchunks)) {
    const uint64_t base = chunk * PER_BLOCK;
    const uint32_t t = (uint32_t)((base >> a.logN) % a.L);
    const TC c = a.tc[t];
    uint64_t s[V][2][4];
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int z = 0; z < 4; ++z) s[v][h][z] = 0;
#pragma unroll 4
    for (uint32_t k = 0; k < a.C; ++k) {
      const uint64_t* __restrict__ p = a.ptrs[k];
      const uint32_t w0 = a.wl[k][t][0], w1 = a.wl[k][t][1];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const u32x4 x = ld<NT>(p + base + 2 * (v * THREADS + threadIdx.x));
        const uint32_t a0 = x.x & M30, a1 = (x.x >> 30) | (x.y << 2);
        const uint32_t b0 = x.z & M30, b1 = (x.z >> 30) | (x.w << 2);
        s[v][0][0] += (uint64_t)a0 * w0;
        s[v][0][1] += (uint64_t)a0 * w1;
        s[v][0][2] += (uint64_t)a1 * w0;
        s[v][0][3] += (uint64_t)a1 * w1;
        s[v][1][0] += (uint64_t)b0 * w0;
        s[v][1][1] += (uint64_t)b0 * w1;
        s[v][1][2] += (uint64_t)b1 * w0;
        s[v][1][3] += (uint64_t)b1 * w1;
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const uint64_t r0 = fold(s[v][0][0], s[v][0][1], s[v][0][2], s[v][0][3], c);
      const uint64_t r1 = fold(s[v][1][0], s[v][1][1], s[v][1][2], s[v][1][3], c);
      u32x4 o;
      o.x = (uint32_t)r0;
      o.y = (uint32_t)(r0 >> 32);
      o.z = (uint32_t)r1;
      o.w = (uint32_t)(r1 >> 32);
      st<NT>(a.out + base + 2 * (v * THREADS + threadIdx.x), o);
    }
    if (!PERSIST) break;
  }
}

// compute-free ceiling: XOR of the learners' vectors (same access pattern)
template <bool NT>
__global__ __launch_bounds__(256) void stream_ceiling(Args a) {
  const uint64_t base = (uint64_t)blockIdx.x * 512;
  u32x4 acc = {0, 0, 0, 0};
#pragma unroll 8
  for (uint32_t k = 0; k < a.C; ++k) acc ^= ld<NT>(a.ptrs[k] + base + 2 * threadIdx.x);
  st<NT>(a.out + base + 2 * threadIdx.x, acc);
}

// single-stream references over learner 0's buffer (same byte count per pass)
template <bool NT>
__global__ __launch_bounds__(256) void copy_ref(const uint64_t* __restrict__ in, uint64_t* __restrict__ out) {
  const uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  st<NT>(out + i, ld<NT>(in + i));
}
template <bool NT>
__global__ __launch_bounds__(256) void read_ref(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                uint64_t n_vec_per_thread, uint64_t stride) {
  const uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  u32x4 acc = {0, 0, 0, 0};
  for (uint64_t k = 0; k < n_vec_per_thread; ++k) acc ^= ld<NT>(in + i + k * stride);
  if (acc.x == 0x12345678u && acc.y == 7u) out[0] = acc.z;  // keep live
}
// ceiling with V vectors per thread per learner
template <int V>
__global__ __launch_bounds__(256) void stream_ceiling_v(Args a) {
  const uint64_t base = (uint64_t)blockIdx.x * 512 * V;
  u32x4 acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = {0, 0, 0, 0};
#pragma unroll 4
  for (uint32_t k = 0; k < a.C; ++k)
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] ^= ld<true>(a.ptrs[k] + base + 2 * (v * 256 + threadIdx.x));
#pragma unroll
  for (int v = 0; v < V; ++v) st<true>(a.out + base + 2 * (v * 256 + threadIdx.x), acc[v]);
}

// learner-interleaved layout: buffer [chunk][C][V*512 residues]; a block reads one
// contiguous C * V * 4 KiB region
template <int V>
__global__ __launch_bounds__(256) void wavg_il(Args a) {
  constexpr uint32_t CH = 512 * V;  // residues per (chunk, learner)
  const uint32_t M30 = (1u << 30) - 1;
  const uint64_t base = (uint64_t)blockIdx.x * CH;           // output residue index
  const uint32_t t = (uint32_t)((base >> a.logN) % a.L);
  const TC c = a.tc[t];
  const uint64_t* __restrict__ src = a.ptrs[0] + (uint64_t)blockIdx.x * CH * a.C;
  uint64_t s[V][2][4];
#pragma unroll
  for (int v = 0; v < V; ++v)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int z = 0; z < 4; ++z) s[v][h][z] = 0;
#pragma unroll 4
  for (uint32_t k = 0; k < a.C; ++k) {
    const uint32_t w0 = a.wl[k][t][0], w1 = a.wl[k][t][1];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const u32x4 x = ld<true>(src + (uint64_t)k * CH + 2 * (v * 256 + threadIdx.x));
      const uint32_t a0 = x.x & M30, a1 = (x.x >> 30) | (x.y << 2);
      const uint32_t b0 = x.z & M30, b1 = (x.z >> 30) | (x.w << 2);
      s[v][0][0] += (uint64_t)a0 * w0;
      s[v][0][1] += (uint64_t)a0 * w1;
      s[v][0][2] += (uint64_t)a1 * w0;
      s[v][0][3] += (uint64_t)a1 * w1;
      s[v][1][0] += (uint64_t)b0 * w0;
      s[v][1][1] += (uint64_t)b0 * w1;
      s[v][1][2] += (uint64_t)b1 * w0;
      s[v][1][3] += (uint64_t)b1 * w1;
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const uint64_t r0 = fold(s[v][0][0], s[v][0][1], s[v][0][2], s[v][0][3], c);
    const uint64_t r1 = fold(s[v][1][0], s[v][1][1], s[v][1][2], s[v][1][3], c);
    u32x4 o;
    o.x = (uint32_t)r0; o.y = (uint32_t)(r0 >> 32); o.z = (uint32_t)r1; o.w = (uint32_t)(r1 >> 32);
    st<true>(a.out + base + 2 * (v * 256 + threadIdx.x), o);
  }
}
// pack per-learner buffers into the interleaved layout (test setup only)
__global__ void pack_il(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint32_t k, uint32_t C,
                        uint32_t CH, uint64_t total) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const uint64_t chunk = i / CH, r = i % CH;
  out[(chunk * C + k) * CH + r] = in[i];
}
extern "C" int wv_pack(const uint64_t* in, uint64_t* out, uint32_t k, uint32_t C, uint32_t CH, uint64_t total) {
  hipLaunchKernelGGL(pack_il, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, 0, in, out, k, C, CH, total);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int V, bool NT, bool PERSIST, int THREADS>
static int launch(const Args& a, int grid_cap, hipStream_t s) {
  constexpr uint32_t PER_BLOCK = 2 * V * THREADS;
  const uint64_t total = a.rows << a.logN;
  const uint64_t nchunks = total / PER_BLOCK;
  uint64_t grid = PERSIST ? (nchunks < (uint64_t)grid_cap ? nchunks : (uint64_t)grid_cap) : nchunks;
  hipLaunchKernelGGL((wavg_v<V, NT, PERSIST, THREADS>), dim3((uint32_t)grid), dim3(THREADS), 0, s,
                     a, nchunks);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int wv_launch(int variant, const Args* a, int grid_cap, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  switch (variant) {
    case 0: return launch<1, true, false, 256>(*a, grid_cap, s);   // product kernel
    case 1: return launch<1, false, false, 256>(*a, grid_cap, s);  // plain loads/stores
    case 2: return launch<2, true, false, 256>(*a, grid_cap, s);   // 4 residues/thread
    case 3: return launch<1, true, true, 256>(*a, grid_cap, s);    // persistent grid-stride
    case 4: return launch<2, true, true, 256>(*a, grid_cap, s);
    case 5: return launch<1, true, false, 512>(*a, grid_cap, s);
    case 6: return launch<4, true, false, 256>(*a, grid_cap, s);
    case 7: return launch<1, true, false, 128>(*a, grid_cap, s);
    case 100: {
      const uint64_t blocks = (a->rows << a->logN) / 512;
      hipLaunchKernelGGL(stream_ceiling<true>, dim3((uint32_t)blocks), dim3(256), 0, s, *a);
      return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    case 101: {
      const uint64_t blocks = (a->rows << a->logN) / 512;
      hipLaunchKernelGGL(stream_ceiling<false>, dim3((uint32_t)blocks), dim3(256), 0, s, *a);
      return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    case 102: case 103: {  // copy: all C learner buffers -> out region sized C*K (use ptrs as a chain)
      const uint64_t blocks = (a->rows << a->logN) / 512;
      for (uint32_t k = 0; k + 1 < a->C; k += 2) {
        if (variant == 102) hipLaunchKernelGGL(copy_ref<true>, dim3((uint32_t)blocks), dim3(256), 0, s, a->ptrs[k], (uint64_t*)a->ptrs[k + 1]);
        else hipLaunchKernelGGL(copy_ref<false>, dim3((uint32_t)blocks), dim3(256), 0, s, a->ptrs[k], (uint64_t*)a->ptrs[k + 1]);
      }
      return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    case 104: {  // read-only, each learner buffer read once, one stream at a time per kernel
      const uint64_t nvec = (a->rows << a->logN) / 2;  // 16B vectors per learner
      const uint64_t per_thr = 16, threads = nvec / per_thr;
      for (uint32_t k = 0; k < a->C; ++k)
        hipLaunchKernelGGL(read_ref<true>, dim3((uint32_t)(threads / 256)), dim3(256), 0, s, a->ptrs[k], a->out, per_thr, threads * 2);
      return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    case 201: case 202: case 204: {  // interleaved; ptrs[0] = packed buffer for that V
      const int V = variant - 200;
      const uint64_t blocks = (a->rows << a->logN) / (512 * V);
      if (V == 1) hipLaunchKernelGGL(wavg_il<1>, dim3((uint32_t)blocks), dim3(256), 0, s, *a);
      if (V == 2) hipLaunchKernelGGL(wavg_il<2>, dim3((uint32_t)blocks), dim3(256), 0, s, *a);
      if (V == 4) hipLaunchKernelGGL(wavg_il<4>, dim3((uint32_t)blocks), dim3(256), 0, s, *a);
      return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    case 105: {
      const uint64_t blocks = (a->rows << a->logN) / 2048;
      hipLaunchKernelGGL(stream_ceiling_v<4>, dim3((uint32_t)blocks), dim3(256), 0, s, *a);
      return hipGetLastError() == hipSuccess ? 0 : -1;
    }
  }
  return -2;
}
extern "C" int wv_sizeof_args() { return (int)sizeof(Args); }
