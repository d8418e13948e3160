// conv_igemm.hip -- implicit-GEMM convolution on the CDNA4 matrix cores.
//
// One kernel serves Conv2D/Conv3D forward (K.layers/convolutional.py:148-182 -> TFB:3128-3165,
// TFB:3277-3314) and, with the flipped/transposed filter, the data gradient of every stride-1 conv.
// GEMM view: M = N*Do*Ho*Wo output pixels, N = Cout, K = taps*Cin (k = tap*Cin + c, channels fastest,
// which is the contiguous axis of the channels-last activations).
//
// Tile: BM x BN outputs per 256-thread workgroup (4 wave64), K staged 128 bytes per row per step
// (64 bf16 / 32 f32) through double-buffered LDS with a 16-byte-chunk XOR swizzle; operands reach the
// MFMA as one 16-byte LDS read per lane per k-group (v_mfma_f32_16x16x32_bf16, or 4x
// v_mfma_f32_16x16x4_f32 in the exact-f32 parity mode).  The operand gather applies, on the fly,
// the BN(+Scale)+ReLU affine of the producing layer, nearest up-sampling, the skip add and zero padding,
// so none of those tensors is ever materialised in HBM.
#include "conv_common.h"
#include "../../include/hdu.h"

// geometry of the fused BN-backward epilogue (epilogue_bn_backward below): thread = (16-byte channel chunk, row lane)
template <typename T, int BM, int BN> struct BnbGeom {
  static constexpr int CH = Chunk<T>::CH;
  static constexpr int NCC = BN / CH;
  static constexpr int NCCP = NCC <= 4 ? 4 : (NCC <= 8 ? 8 : (NCC <= 16 ? 16 : 32));
  static constexpr int RSTEP = 256 / NCCP;
  static constexpr int IT = (BM + RSTEP - 1) / RSTEP;
  static constexpr bool EARLY = IT <= 8;             // the u / old-gradient chunks of a thread fit in registers
  static_assert(NCC <= 32, "tile shape");
};

template <bool SPLIT, typename T, int BM, int BN, int WAVES_M, int WAVES_N>
__device__ __forceinline__ void conv_igemm_body(const ConvK& p, char* smem) {
  constexpr int CH = Chunk<T>::CH;
  constexpr int BK = 8 * CH;
  constexpr int A_IT = BM / 32;
  constexpr int B_IT = (BN + 31) / 32;
  constexpr int WM = BM / WAVES_M;
  constexpr int WN = BN / WAVES_N;
  constexpr int TM = WM / 16;
  constexpr int TN = WN / 16;
  constexpr int STAGE = (BM + BN) * 128;
  static_assert(WAVES_M * WAVES_N == 4, "4 waves");
  static_assert(BM % 32 == 0 && WM % 16 == 0 && WN % 16 == 0, "tile");


  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;
  const int kc = tid & 7;
  const int r0 = tid >> 3;
  const long long m0 = (long long)((p.xcd_swizzle & 1) ? xcd_tile_index(blockIdx.x, gridDim.x) : blockIdx.x) * BM;
  const int n0 = blockIdx.y * BN;
  const T* __restrict__ xp = (const T*)p.x;
  const T* __restrict__ sp = (const T*)p.skip;
  const T* __restrict__ wp = (const T*)p.w;
  const bool has_pro = p.pro_a != nullptr;
  const bool has_skip = p.skip != nullptr;

  // ---- per-row (output pixel) state, fixed for the whole K loop ----
  // rpix = pixel index of the tap-(0,0,0) input position (may be "negative"; only used when in bounds)
  const bool ups = (p.ud | p.uh | p.uw) != 0;
  int rn[A_IT], rid[A_IT], rih[A_IT], riw[A_IT], rpix[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const long long m = m0 + r0 + i * 32;
    if (m < p.M) {
      const unsigned mu = (unsigned)m;                    // M < 2^31 (checked on the host): 32-bit divisions
      const int ow = (int)(mu % (unsigned)p.Wo);
      unsigned t = mu / (unsigned)p.Wo;
      const int oh = (int)(t % (unsigned)p.Ho);
      t /= (unsigned)p.Ho;
      const int od = (int)(t % (unsigned)p.Do);
      rn[i] = (int)(t / (unsigned)p.Do);
      rid[i] = od * p.sd - p.pd;
      rih[i] = oh * p.sh - p.ph;
      riw[i] = ow * p.sw - p.pw;
      rpix[i] = ((rn[i] * p.De + rid[i]) * p.He + rih[i]) * p.We + riw[i];
    } else {
      rn[i] = 0;
      rid[i] = -(1 << 28);
      rih[i] = -(1 << 28);
      riw[i] = -(1 << 28);
      rpix[i] = 0;
    }
  }

  // ---- per-thread k state: this thread always stages 16-byte chunk `kc` of the K tile ----
  int k = kc * CH;
  int tap_i = 0;
  int c, kd, kh, kw;
  {
    const int tap = k / p.Cin;
    c = k - tap * p.Cin;
    kw = tap % p.KW;
    const int t = tap / p.KW;
    kh = t % p.KH;
    kd = t / p.KH;
  }

  u32x4 areg[A_IT], sreg[A_IT], breg[B_IT];
  float pa[CH], pb[CH];
  unsigned okmask = 0;

  auto load_tile = [&]() {
    okmask = 0;
    const bool kvalid = kd < p.KD;
    const int tapoff = (kd * p.He + kh) * p.We + kw;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int id = rid[i] + kd, ih = rih[i] + kh, iw = riw[i] + kw;
      const bool ok = kvalid && (unsigned)id < (unsigned)p.De && (unsigned)ih < (unsigned)p.He &&
                      (unsigned)iw < (unsigned)p.We;
      u32x4 v = {0u, 0u, 0u, 0u};
      u32x4 s = {0u, 0u, 0u, 0u};
      if (ok) {
        const int e = rpix[i] + tapoff;   // effective-resolution pixel index
        const int src = ups ? ((rn[i] * p.Di + (id >> p.ud)) * p.Hi + (ih >> p.uh)) * p.Wi + (iw >> p.uw) : e;
        v = *(const u32x4*)(xp + (long long)src * p.ldx + c);
        if (has_skip) s = *(const u32x4*)(sp + (long long)e * p.ldskip + c);
        okmask |= 1u << i;
      }
      areg[i] = v;
      sreg[i] = s;
    }
    if (has_pro && kvalid) {
#pragma unroll
      for (int j = 0; j < CH; j += 4) {
        const f32x4 a4 = *(const f32x4*)(p.pro_a + c + j);
        const f32x4 b4 = *(const f32x4*)(p.pro_b + c + j);
        pa[j] = a4.x; pa[j + 1] = a4.y; pa[j + 2] = a4.z; pa[j + 3] = a4.w;
        pb[j] = b4.x; pb[j + 1] = b4.y; pb[j + 2] = b4.z; pb[j + 3] = b4.w;
      }
    }
#pragma unroll
    for (int j = 0; j < B_IT; ++j) {
      const int row = r0 + j * 32;
      const int col = n0 + row;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (row < BN && col < p.Cout && k < p.Ktot) v = *(const u32x4*)(wp + (long long)col * p.Ktot + k);
      breg[j] = v;
    }
  };

  auto store_tile = [&](int buf) {
    char* As = smem + buf * STAGE;
    char* Bs = As + BM * 128;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      u32x4 v = areg[i];
      if ((has_pro || has_skip) && ((okmask >> i) & 1u)) {
        float f[CH], g[CH];
        Chunk<T>::unpack(v, f);
        if (has_pro) {
#pragma unroll
          for (int j = 0; j < CH; ++j) {
            f[j] = pa[j] * f[j] + pb[j];
            if (p.pro_relu) f[j] = f[j] > 0.f ? f[j] : 0.f;
          }
        }
        if (has_skip) {
          Chunk<T>::unpack(sreg[i], g);
#pragma unroll
          for (int j = 0; j < CH; ++j) f[j] += g[j];
        }
        v = Chunk<T>::pack(f);
      }
      *(u32x4*)(As + lds_chunk_off(r0 + i * 32, kc)) = v;
    }
#pragma unroll
    for (int j = 0; j < B_IT; ++j) {
      const int row = r0 + j * 32;
      if (row < BN) *(u32x4*)(Bs + lds_chunk_off(row, kc)) = breg[j];
    }
  };

  auto advance = [&]() {
    k += BK;
    c += BK;
    while (c >= p.Cin) {
      c -= p.Cin;
      ++tap_i;
      if (++kw == p.KW) {
        kw = 0;
        if (++kh == p.KH) {
          kh = 0;
          ++kd;
        }
      }
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (p.Ktot + BK - 1) / BK;
  load_tile();
  store_tile(0);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) {
      advance();
      load_tile();
    }
    {
      const char* As = smem + buf * STAGE;
      const char* Bs = As + BM * 128;
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        u32x4 af[TM], bf[TN];
        const int chunk = kg * 4 + (lane >> 4);
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = *(const u32x4*)(As + lds_chunk_off(wm * WM + i * 16 + (lane & 15), chunk));
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = *(const u32x4*)(Bs + lds_chunk_off(wn * WN + j * 16 + (lane & 15), chunk));
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = Mma<T>::template kgroup<SPLIT>(bf[j], af[i], acc[i][j]);   // transposed tile: see igemm_epilogue
      }
    }
    if (more) store_tile(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: bias, dropout, optional accumulate, store ----
  u32x4 no_uv[BnbGeom<T, BM, BN>::EARLY ? BnbGeom<T, BM, BN>::IT : 1], no_ov[BnbGeom<T, BM, BN>::EARLY ? BnbGeom<T, BM, BN>::IT : 1];
  igemm_epilogue<T, BM, BN, WM, WN, TM, TN, 2 * STAGE, false>(p, acc, smem, m0, n0, wm, wn, lane, tid, no_uv, no_ov, false);
}

// the float32 instantiations carry both contraction forms (ConvK::f32_split, Mma<float>): one uniform branch at entry
template <typename T, int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(256) void conv_igemm_kernel(ConvK p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * (BM + BN) * 128];
  if constexpr (sizeof(T) == 4) {
    if (p.f32_split) { conv_igemm_body<true, T, BM, BN, WAVES_M, WAVES_N>(p, smem); return; }
  }
  conv_igemm_body<false, T, BM, BN, WAVES_M, WAVES_N>(p, smem);
}

// =====================================================================================
// filter gradient.  GEMM view: rows = Cout, cols = k (tap*Cin + c), contraction over output pixels.
// Both operands are channel-contiguous in HBM but the MFMA wants them pixel-contiguous per lane, so the
// staging pass transposes on the way into LDS ([channel][pixel] tiles, same 128-byte rows / swizzle).
// The pixel range is split across blockIdx.z; partial results are accumulated with float atomics.
__device__ __forceinline__ int wg_swz(int row) { return (row ^ (row >> 3)) & 7; }

template <bool SPLIT, typename T, int BCO>
__device__ __forceinline__ void conv_wgrad_body(const ConvK& p, float* __restrict__ dw, long long rows_per_split, char* smem) {
  constexpr int CH = Chunk<T>::CH;
  constexpr int PX = 8 * CH;          // pixels per step = elements per 128-byte LDS row
  constexpr int BKC = 128;            // k columns per workgroup
  constexpr int NCC = BKC / CH;       // 16-byte chunk columns of the x tile
  constexpr int X_IT = PX * NCC / 256;
  constexpr int NDC = BCO / CH;       // chunk columns of the dy tile
  constexpr int D_IT = (PX * NDC + 255) / 256;
  constexpr int TM = BCO / 16;
  constexpr int TN = 2;
  constexpr int STAGE = (BCO + BKC) * 128;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const T* __restrict__ xp = (const T*)p.x;
  const T* __restrict__ sp = (const T*)p.skip;
  const T* __restrict__ dyp = (const T*)p.y;
  const bool has_pro = p.pro_a != nullptr;
  const bool has_skip = p.skip != nullptr;

  const int kcol0 = blockIdx.x * BKC;
  const int co0 = blockIdx.y * BCO;
  const long long m_begin = (long long)blockIdx.z * rows_per_split;
  long long m_end = m_begin + rows_per_split;
  if (m_end > p.M) m_end = p.M;

  // ---- fixed k column of this thread (x tile) ----
  const int kcc = tid % NCC;
  const int pxl = tid / NCC;
  const int kk = kcol0 + kcc * CH;
  const bool kvalid = kk < p.Ktot;
  int c = 0, kd = 0, kh = 0, kw = 0;
  if (kvalid) {
    const int tap = kk / p.Cin;
    c = kk - tap * p.Cin;
    kw = tap % p.KW;
    const int t = tap / p.KW;
    kh = t % p.KH;
    kd = t / p.KH;
  }
  float pa[CH], pb[CH];
  if (has_pro && kvalid) {
#pragma unroll
    for (int j = 0; j < CH; ++j) { pa[j] = p.pro_a[c + j]; pb[j] = p.pro_b[c + j]; }
  }
  // ---- per pixel-slot state (x tile) ----
  int sn[X_IT], sod[X_IT], soh[X_IT], sow[X_IT];
#pragma unroll
  for (int i = 0; i < X_IT; ++i) {
    const long long m = m_begin + pxl + i * (256 / NCC);
    const unsigned mu = (unsigned)m;                      // M < 2^31 (checked on the host): 32-bit divisions
    const int ow = (int)(mu % (unsigned)p.Wo);
    unsigned t = mu / (unsigned)p.Wo;
    const int oh = (int)(t % (unsigned)p.Ho);
    t /= (unsigned)p.Ho;
    sod[i] = (int)(t % (unsigned)p.Do);
    sn[i] = (int)(t / (unsigned)p.Do);
    soh[i] = oh;
    sow[i] = ow;
  }

  u32x4 xreg[X_IT], sreg[X_IT], dreg[D_IT];
  unsigned okmask = 0;

  auto load_tile = [&](long long mt) {
    okmask = 0;
#pragma unroll
    for (int i = 0; i < X_IT; ++i) {
      const long long m = mt + pxl + i * (256 / NCC);
      const int id = sod[i] * p.sd - p.pd + kd, ih = soh[i] * p.sh - p.ph + kh, iw = sow[i] * p.sw - p.pw + kw;
      const bool ok = kvalid && m < m_end && (unsigned)id < (unsigned)p.De && (unsigned)ih < (unsigned)p.He &&
                      (unsigned)iw < (unsigned)p.We;
      u32x4 v = {0u, 0u, 0u, 0u};
      u32x4 s = {0u, 0u, 0u, 0u};
      if (ok) {
        const long long src =
            (((long long)sn[i] * p.Di + (id >> p.ud)) * p.Hi + (ih >> p.uh)) * p.Wi + (iw >> p.uw);
        v = *(const u32x4*)(xp + src * p.ldx + c);
        if (has_skip) {
          const long long e = (((long long)sn[i] * p.De + id) * p.He + ih) * p.We + iw;
          s = *(const u32x4*)(sp + e * p.ldskip + c);
        }
        okmask |= 1u << i;
      }
      xreg[i] = v;
      sreg[i] = s;
    }
#pragma unroll
    for (int j = 0; j < D_IT; ++j) {
      const int q = tid + j * 256;
      const int dcc = q % NDC;
      const int dpx = q / NDC;
      const long long m = mt + dpx;
      const int co = co0 + dcc * CH;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (dpx < PX && m < m_end && co < p.Cout) v = *(const u32x4*)(dyp + m * p.ldy + co);
      dreg[j] = v;
    }
  };

  auto advance_pixels = [&]() {
#pragma unroll
    for (int i = 0; i < X_IT; ++i) {
      sow[i] += PX;
      while (sow[i] >= p.Wo) {
        sow[i] -= p.Wo;
        if (++soh[i] == p.Ho) {
          soh[i] = 0;
          if (++sod[i] == p.Do) {
            sod[i] = 0;
            ++sn[i];
          }
        }
      }
    }
  };

  auto store_tile = [&](int buf) {
    char* At = smem + buf * STAGE;       // [BCO][PX]  dy^T
    char* Bt = At + BCO * 128;           // [BKC][PX]  x_eff^T
#pragma unroll
    for (int i = 0; i < X_IT; ++i) {
      float f[CH];
      Chunk<T>::unpack(xreg[i], f);
      if ((okmask >> i) & 1u) {
        if (has_pro) {
#pragma unroll
          for (int j = 0; j < CH; ++j) {
            f[j] = pa[j] * f[j] + pb[j];
            if (p.pro_relu) f[j] = f[j] > 0.f ? f[j] : 0.f;
          }
        }
        if (has_skip) {
          float g[CH];
          Chunk<T>::unpack(sreg[i], g);
#pragma unroll
          for (int j = 0; j < CH; ++j) f[j] += g[j];
        }
      }
      const int px = pxl + i * (256 / NCC);
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int row = kcc * CH + j;
        T* q = (T*)(Bt + row * 128 + (((px / CH) ^ wg_swz(row)) << 4)) + (px % CH);
        Chunk<T>::store1(q, f[j]);
      }
    }
#pragma unroll
    for (int jj = 0; jj < D_IT; ++jj) {
      const int q = tid + jj * 256;
      const int dcc = q % NDC;
      const int dpx = q / NDC;
      if (dpx < PX) {
        float f[CH];
        Chunk<T>::unpack(dreg[jj], f);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int row = dcc * CH + j;
          T* qq = (T*)(At + row * 128 + (((dpx / CH) ^ wg_swz(row)) << 4)) + (dpx % CH);
          Chunk<T>::store1(qq, f[j]);
        }
      }
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nsteps = (int)((m_end - m_begin + PX - 1) / PX);
  if (nsteps > 0) {
    load_tile(m_begin);
    store_tile(0);
  }
  __syncthreads();
  for (int st = 0; st < nsteps; ++st) {
    const int buf = st & 1;
    const bool more = st + 1 < nsteps;
    if (more) {
      advance_pixels();
      load_tile(m_begin + (long long)(st + 1) * PX);
    }
    {
      const char* At = smem + buf * STAGE;
      const char* Bt = At + BCO * 128;
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        u32x4 af[TM], bf[TN];
        const int chunk = kg * 4 + (lane >> 4);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int row = i * 16 + (lane & 15);
          af[i] = *(const u32x4*)(At + row * 128 + ((chunk ^ wg_swz(row)) << 4));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int row = wave * 32 + j * 16 + (lane & 15);
          bf[j] = *(const u32x4*)(Bt + row * 128 + ((chunk ^ wg_swz(row)) << 4));
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = Mma<T>::template kgroup<SPLIT>(af[i], bf[j], acc[i][j]);
      }
    }
    if (more) store_tile(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + i * 16 + (lane >> 4) * 4 + r;
      if (co >= p.Cout) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int kcol = kcol0 + wave * 32 + j * 16 + (lane & 15);
        if (kcol < p.Ktot) atomicAdd(dw + (long long)co * p.Ktot + kcol, acc[i][j][r]);
      }
    }
}

// the float32 instantiations carry both contraction forms (ConvK::f32_split, Mma<float>): one uniform branch at entry
template <typename T, int BCO>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(ConvK p, float* __restrict__ dw, long long rows_per_split) {
  __shared__ __attribute__((aligned(16))) char smem[2 * (BCO + 128) * 128];
  if constexpr (sizeof(T) == 4) {
    if (p.f32_split) { conv_wgrad_body<true, T, BCO>(p, dw, rows_per_split, smem); return; }
  }
  conv_wgrad_body<false, T, BCO>(p, dw, rows_per_split, smem);
}

// =====================================================================================
// bf16 filter gradient, transpose-read form.  Same GEMM view as conv_wgrad_kernel, but the staging pass stores the
// channel-contiguous 16-byte chunks as they come ([pixel][channel] LDS tiles, one ds_write_b128 per chunk) and the
// MFMA operands (8 consecutive pixels of one channel per lane) are produced by ds_read_b64_tr_b16.
// 32-byte segments of each tile row are XOR-swizzled with the pixel index so that the 8 rows a 32-lane pass touches
// fall on distinct banks.
template <int ROWB>
__device__ __forceinline__ int tr_off(int px, int byte_col) {
  int seg = byte_col >> 5;
  if (ROWB == 256) seg ^= (px & 3) | ((px >> 1) & 4);
  else seg ^= ((px >> 1) & 1) | (((px >> 3) & 1) << 1);
  return px * ROWB + (seg << 5) + (byte_col & 31);
}

template <int BCO>
__global__ __launch_bounds__(256) void conv_wgrad_tr_kernel(ConvK p, float* __restrict__ dw, long long rows_per_split) {
  typedef bf16_t T;
  constexpr int CH = 8;
  constexpr int PX = 64;              // pixels per step (two MFMA k-groups of 32)
  constexpr int BKC = 128;            // k columns per workgroup
  constexpr int XROWB = BKC * 2;      // 256 B per pixel row of the x tile
  constexpr int DROWB = 128;          // dy tile row: up to 64 output channels
  constexpr int NDC = BCO / CH;
  constexpr int D_IT = (PX * NDC + 255) / 256;
  constexpr int TM = BCO / 16;
  constexpr int TN = 2;
  constexpr int STAGE = PX * (XROWB + DROWB);
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const T* __restrict__ xp = (const T*)p.x;
  const T* __restrict__ sp = (const T*)p.skip;
  const T* __restrict__ dyp = (const T*)p.y;
  const bool has_pro = p.pro_a != nullptr;
  const bool has_skip = p.skip != nullptr;
  const bool ups = (p.ud | p.uh | p.uw) != 0;

  const int kcol0 = blockIdx.x * BKC;
  const int co0 = blockIdx.y * BCO;
  const long long m_begin = (long long)blockIdx.z * rows_per_split;
  long long m_end = m_begin + rows_per_split;
  if (m_end > p.M) m_end = p.M;

  const int kcc = tid & 15;
  const int pxl = tid >> 4;           // 0..15; pixel slots pxl + 16*i
  const int kk = kcol0 + kcc * CH;
  const bool kvalid = kk < p.Ktot;
  int c = 0, kd = 0, kh = 0, kw = 0;
  if (kvalid) {
    const int tap = kk / p.Cin;
    c = kk - tap * p.Cin;
    kw = tap % p.KW;
    const int t = tap / p.KW;
    kh = t % p.KH;
    kd = t / p.KH;
  }
  float pa[CH], pb[CH];
  if (has_pro && kvalid) {
#pragma unroll
    for (int j = 0; j < CH; ++j) { pa[j] = p.pro_a[c + j]; pb[j] = p.pro_b[c + j]; }
  }
  int sn[4], sod[4], soh[4], sow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long m = m_begin + pxl + i * 16;
    const unsigned mu = (unsigned)m;                      // M < 2^31 (checked on the host): 32-bit divisions
    const int ow = (int)(mu % (unsigned)p.Wo);
    unsigned t = mu / (unsigned)p.Wo;
    const int oh = (int)(t % (unsigned)p.Ho);
    t /= (unsigned)p.Ho;
    sod[i] = (int)(t % (unsigned)p.Do);
    sn[i] = (int)(t / (unsigned)p.Do);
    soh[i] = oh;
    sow[i] = ow;
  }

  u32x4 xreg[4], sreg[4], dreg[D_IT];
  unsigned okmask = 0;

  auto load_tile = [&](long long mt) {
    okmask = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long m = mt + pxl + i * 16;
      const int id = sod[i] * p.sd - p.pd + kd, ih = soh[i] * p.sh - p.ph + kh, iw = sow[i] * p.sw - p.pw + kw;
      const bool ok = kvalid && m < m_end && (unsigned)id < (unsigned)p.De && (unsigned)ih < (unsigned)p.He &&
                      (unsigned)iw < (unsigned)p.We;
      u32x4 v = {0u, 0u, 0u, 0u};
      u32x4 s = {0u, 0u, 0u, 0u};
      if (ok) {
        const int e = ((sn[i] * p.De + id) * p.He + ih) * p.We + iw;
        const int src = ups ? ((sn[i] * p.Di + (id >> p.ud)) * p.Hi + (ih >> p.uh)) * p.Wi + (iw >> p.uw) : e;
        v = *(const u32x4*)(xp + (long long)src * p.ldx + c);
        if (has_skip) s = *(const u32x4*)(sp + (long long)e * p.ldskip + c);
        okmask |= 1u << i;
      }
      xreg[i] = v;
      sreg[i] = s;
    }
#pragma unroll
    for (int j = 0; j < D_IT; ++j) {
      const int q = tid + j * 256;
      const int dcc = q % NDC;
      const int dpx = q / NDC;
      const long long m = mt + dpx;
      const int co = co0 + dcc * CH;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (dpx < PX && m < m_end && co < p.Cout) v = *(const u32x4*)(dyp + m * p.ldy + co);
      dreg[j] = v;
    }
  };

  auto advance_pixels = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sow[i] += PX;
      while (sow[i] >= p.Wo) {
        sow[i] -= p.Wo;
        if (++soh[i] == p.Ho) {
          soh[i] = 0;
          if (++sod[i] == p.Do) {
            sod[i] = 0;
            ++sn[i];
          }
        }
      }
    }
  };

  auto store_tile = [&](int buf) {
    char* Xt = smem + buf * STAGE;       // [PX][BKC] x_eff
    char* Dt = Xt + PX * XROWB;          // [PX][<=64] dy
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 v = xreg[i];
      if ((has_pro || has_skip) && ((okmask >> i) & 1u)) {
        float f[CH];
        Chunk<T>::unpack(v, f);
        if (has_pro) {
#pragma unroll
          for (int j = 0; j < CH; ++j) {
            f[j] = pa[j] * f[j] + pb[j];
            if (p.pro_relu) f[j] = f[j] > 0.f ? f[j] : 0.f;
          }
        }
        if (has_skip) {
          float g[CH];
          Chunk<T>::unpack(sreg[i], g);
#pragma unroll
          for (int j = 0; j < CH; ++j) f[j] += g[j];
        }
        v = Chunk<T>::pack(f);
      }
      const int px = pxl + i * 16;
      *(u32x4*)(Xt + tr_off<XROWB>(px, kcc * 16)) = v;
    }
#pragma unroll
    for (int jj = 0; jj < D_IT; ++jj) {
      const int q = tid + jj * 256;
      const int dcc = q % NDC;
      const int dpx = q / NDC;
      if (dpx < PX) *(u32x4*)(Dt + tr_off<DROWB>(dpx, dcc * 16)) = dreg[jj];
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nsteps = (int)((m_end - m_begin + PX - 1) / PX);
  if (nsteps > 0) {
    load_tile(m_begin);
    store_tile(0);
  }
  __syncthreads();
  const int li = lane & 15, lg = lane >> 4;
  for (int st = 0; st < nsteps; ++st) {
    const int buf = st & 1;
    const bool more = st + 1 < nsteps;
    if (more) {
      advance_pixels();
      load_tile(m_begin + (long long)(st + 1) * PX);
    }
    {
      const char* Xt = smem + buf * STAGE;
      const char* Dt = Xt + PX * XROWB;
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        u32x4 af[TM], bf[TN];
        const int prow = kg * 32 + lg * 8 + (li >> 2);   // pixel row this lane addresses (first half)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int bc = (i * 16 + (li & 3) * 4) * 2;
          const u32x2 lo = hdu_lds_tr16_b64(Dt + tr_off<DROWB>(prow, bc));
          const u32x2 hi = hdu_lds_tr16_b64(Dt + tr_off<DROWB>(prow + 4, bc));
          af[i] = u32x4{lo.x, lo.y, hi.x, hi.y};
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int bc = (wave * 32 + j * 16 + (li & 3) * 4) * 2;
          const u32x2 lo = hdu_lds_tr16_b64(Xt + tr_off<XROWB>(prow, bc));
          const u32x2 hi = hdu_lds_tr16_b64(Xt + tr_off<XROWB>(prow + 4, bc));
          bf[j] = u32x4{lo.x, lo.y, hi.x, hi.y};
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = Mma<T>::template kgroup<false>(af[i], bf[j], acc[i][j]);
      }
    }
    if (more) store_tile(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + i * 16 + (lane >> 4) * 4 + r;
      if (co >= p.Cout) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int kcol = kcol0 + wave * 32 + j * 16 + (lane & 15);
        if (kcol < p.Ktot) atomicAdd(dw + (long long)co * p.Ktot + kcol, acc[i][j][r]);
      }
    }
}

#ifdef HDU_TIMELINE
#define HDU_TL_WGS 8192
__device__ unsigned long long hdu_timeline[HDU_TL_WGS * 10];
#define HDU_TP(i)                                                                                               \
  do {                                                                                                           \
    if (threadIdx.x == 0) {                                                                                      \
      const unsigned b_ = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;                        \
      if (b_ < HDU_TL_WGS) {                                                                                     \
        hdu_timeline[b_ * 10 + (i)] = __builtin_readcyclecounter();                                              \
        if ((i) == 0) hdu_timeline[b_ * 10 + 8] = wall_clock64();                                                \
        if ((i) >= 5) hdu_timeline[b_ * 10 + 9] = wall_clock64();                                                \
      }                                                                                                          \
    }                                                                                                            \
  } while (0)
extern "C" int hdu_timeline_read(unsigned long long* host, int clear) {
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(hdu_timeline), sizeof(unsigned long long) * HDU_TL_WGS * 10) != hipSuccess) return 1;
  if (clear) {
    void* dp = nullptr;
    if (hipGetSymbolAddress(&dp, HIP_SYMBOL(hdu_timeline)) != hipSuccess) return 1;
    if (hipMemset(dp, 0, sizeof(unsigned long long) * HDU_TL_WGS * 10) != hipSuccess) return 1;
  }
  return 0;
}
#else
#define HDU_TP(i) do { } while (0)
#endif

// ---- per-channel moments of the output tile while it is still staged in LDS (ConvK::stats_partial).  Called by all
// 256 threads after the tile stores; reads the tile only.  Thread = (16-byte column chunk, row lane): the 16 row lanes of
// a chunk are 16 ADJACENT lanes of a wave, each sums rows rl, rl+16, ... in registers, a 4-step xor butterfly adds the 16
// lanes, and lane 0 of the group adds the chunk's 2*CH totals to this workgroup's slot row with global float atomics
// (no LDS scratch, no extra barrier; LDS float atomics on a shared column were measured far slower).
template <typename T, int BM, int BN, int ROWB, typename RowValid>
__device__ __forceinline__ void epilogue_stats(const ConvK& p, char* smem, int n0, int tid, unsigned slot, RowValid valid) {
  constexpr int CH = Chunk<T>::CH;
  constexpr int NCC = BN / CH;
  float* dst = p.stats_partial + (long long)(slot % (unsigned)p.stats_slots) * 2 * p.Cout;
  const int rl = tid & 15;
#pragma unroll
  for (int it = 0; it < (NCC + 15) / 16; ++it) {      // every lane takes every trip (the butterfly is wave-wide)
    const int cc = (tid >> 4) + it * 16;
    const int nbase = n0 + cc * CH;
    float s1[CH], s2[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    float sh[CH];
    {
      const int nc = (cc < NCC && nbase < p.Cout) ? nbase : 0;      // unconditional, clamped (see igemm_epilogue)
#pragma unroll
      for (int j = 0; j < CH; j += 4) {
        const f32x4 v4 = *(const f32x4*)(p.stats_shift + nc + j);
        sh[j] = v4[0]; sh[j + 1] = v4[1]; sh[j + 2] = v4[2]; sh[j + 3] = v4[3];
      }
    }
    {
      // every row of the lane requested up front, unconditionally (a chunk beyond the tile re-reads chunk 0; rows past M and
      // lanes without a column are masked in the arithmetic): the per-row `continue` of round 2 made this a chain of BM / 16
      // dependent LDS round trips -- measured round 3 (profiles/r03_timeline_epilogue_split.txt): the statistics cost 2.1 us
      // of a 128x96 tile's 4.7 us epilogue
      const bool col = cc < NCC && nbase < p.Cout;
      const int ccq = col ? cc : 0;
      u32x4 rv[BM / 16];
#pragma unroll
      for (int q = 0; q < BM / 16; ++q) rv[q] = *(const u32x4*)(smem + (rl + q * 16) * ROWB + ccq * 16);
#pragma unroll
      for (int q = 0; q < BM / 16; ++q) {
        const float keep = (col && valid(rl + q * 16)) ? 1.f : 0.f;
        float f[CH];
        Chunk<T>::unpack(rv[q], f);
#pragma unroll
        for (int j = 0; j < CH; ++j) { const float d = (f[j] - sh[j]) * keep; s1[j] += d; s2[j] += d * d; }
      }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) { s1[j] = hdu_row16_sum(s1[j]); s2[j] = hdu_row16_sum(s2[j]); }
    // every lane of the 16-lane group holds all 2 * CH totals: lane q adds total q (q < CH: sum of channel q, else the sum of
    // squares of channel q - CH) -- ONE atomic instruction per wave with 64 different addresses instead of 2 * CH
    // instructions with 4 active lanes each
    float mine = 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      mine = rl == j ? s1[j] : mine;
      mine = rl == CH + j ? s2[j] : mine;
    }
    if (rl < 2 * CH && cc < NCC && nbase < p.Cout)
      atomicAdd(dst + (rl < CH ? 0 : p.Cout) + nbase + (rl < CH ? rl : rl - CH), mine);
  }
}

// ---- fused BatchNormalization(+Scale)+ReLU backward of a data-gradient launch (ConvK::bnb_*, include/hdu.h).  The staged
// tile is dz; each thread owns ONE 16-byte channel chunk (coefficients in registers) and walks the tile rows, so that
// consecutive lanes store consecutive chunks of a row (full 128-byte lines) and a thread's S1 / S2 partial sums stay in
// registers; lanes that share a chunk meet in a wave butterfly, the four waves in LDS, and one lane per channel adds
// the workgroup's sums to a slot row with float atomics.

// issues the thread's u (and, in accumulate mode, old-gradient) loads: called BEFORE the accumulators are staged through
// LDS, so that their latency hides behind the two barriers and the staging pass instead of standing in the epilogue
template <typename T, int BM, int BN, int NIT>
__device__ __forceinline__ void bnb_issue_loads(const ConvK& p, long long m0, int n0, int tid, int it0, u32x4 (&uv)[NIT],
                                                u32x4 (&ov)[NIT]) {
  typedef BnbGeom<T, BM, BN> G;
  const int cc = tid % G::NCCP, r0 = tid / G::NCCP;
  const int n = n0 + cc * G::CH;
  const bool col_ok = cc < G::NCC && n < p.Cout;
  const T* __restrict__ up = (const T*)p.bnb_u;
  const T* __restrict__ yp = (const T*)p.y;
#pragma unroll
  for (int q = 0; q < NIT; ++q) {
    const int row = r0 + (it0 + q) * G::RSTEP;
    const long long m = m0 + row;
    const bool ok = col_ok && row < BM && m < p.M;
    // UNCONDITIONAL loads (a lane without work re-reads element 0 of the tensor and ignores it): a per-lane
    // "load or zero" select makes hipcc branch around every load and wait vmcnt(0) behind it -- measured in the ISA of
    // round 2's build: one full memory round trip per chunk, 4-8 of them in a row per tile epilogue
    uv[q] = *(const u32x4*)(up + (ok ? m * p.bnb_ldu + n : 0));
    ov[q] = *(const u32x4*)(yp + ((ok && p.accumulate) ? m * p.ldy + n : 0));
  }
}

template <typename T, int BM, int BN, int ROWB>
__device__ __forceinline__ void epilogue_bn_backward(const ConvK& p, char* smem, long long m0, int n0, int tid,
                                                     u32x4 (&pre_uv)[BnbGeom<T, BM, BN>::EARLY ? BnbGeom<T, BM, BN>::IT : 1],
                                                     u32x4 (&pre_ov)[BnbGeom<T, BM, BN>::EARLY ? BnbGeom<T, BM, BN>::IT : 1]) {
  typedef BnbGeom<T, BM, BN> G;
  constexpr int CH = G::CH, NCC = G::NCC, NCCP = G::NCCP, RSTEP = G::RSTEP, IT = G::IT;
  constexpr int UNR = G::EARLY ? IT : 4;
  static_assert(IT % UNR == 0, "tile shape");
  const int cc = tid % NCCP, r0 = tid / NCCP;
  const int n = n0 + cc * CH;
  const bool col_ok = cc < NCC && n < p.Cout;
  const bool sums = p.bnb_partial != nullptr;
  const bool relu = (p.bnb_relu & 1) != 0, from_z = (p.bnb_relu & 2) != 0;
  // bit 2 (round 6): SUMS ONLY -- the tile is stored as raw dz (the apply pass that follows, hdu_bn_bwd_apply_sums, needs it), the
  // epilogue only contributes S1 / S2: the separate reduction pass over (dz, u) of a batch-statistics BN goes
  const bool raw = (p.bnb_relu & 4) != 0;
  float a[CH], b[CH], mu[CH], rs[CH], s1[CH], s2[CH];
  {
    // unconditional vector loads at a clamped channel index (see bnb_issue_loads): four loads in flight together instead
    // of 4 x CH branch + wait sequences; values of lanes without a column are never used
    const int nc = col_ok ? n : 0;
    const float* pmu = sums ? p.bnb_mean : p.bnb_a;
    const float* prs = sums ? p.bnb_rstd : p.bnb_a;
#pragma unroll
    for (int j = 0; j < CH; j += 4) {
      const f32x4 va = *(const f32x4*)(p.bnb_a + nc + j), vb = *(const f32x4*)(p.bnb_b + nc + j);
      const f32x4 vm = *(const f32x4*)(pmu + nc + j), vr = *(const f32x4*)(prs + nc + j);
#pragma unroll
      for (int r = 0; r < 4; ++r) { a[j + r] = va[r]; b[j + r] = vb[r]; mu[j + r] = sums ? vm[r] : 0.f; rs[j + r] = sums ? vr[r] : 0.f; }
    }
    if (from_z) {
      // bnb_u holds z = relu(a*u + b): the normalised input is (u - mean) * rstd = (z - (b + a*mean)) * (rstd / a) wherever z > 0,
      // the only elements that count (a channel with a == 0 has no recoverable input: its S2 stays 0)
#pragma unroll
      for (int j = 0; j < CH; ++j) { mu[j] = b[j] + a[j] * mu[j]; rs[j] = a[j] != 0.f ? rs[j] / a[j] : 0.f; }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
  }
  T* __restrict__ yp = (T*)p.y;
  for (int it0 = 0; it0 < IT; it0 += UNR) {
    u32x4 luv[UNR], lov[UNR];
    if constexpr (!G::EARLY) {
      bnb_issue_loads<T, BM, BN, UNR>(p, m0, n0, tid, it0, luv, lov);
      HDU_SCHED_BARRIER();
    }
#pragma unroll
    for (int q = 0; q < UNR; ++q) {
      const int row = r0 + (it0 + q) * RSTEP;
      if (!(col_ok && row < BM && m0 + row < p.M)) continue;
      float dz[CH], u[CH], o[CH];
      Chunk<T>::unpack(*(const u32x4*)(smem + row * ROWB + cc * 16), dz);
      u32x4 uq, oq;
      if constexpr (G::EARLY) { uq = pre_uv[q]; oq = pre_ov[q]; } else { uq = luv[q]; oq = lov[q]; }
      Chunk<T>::unpack(uq, u);
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const float sj = from_z ? u[j] : a[j] * u[j] + b[j];
        const float g = (!relu || sj > 0.f) ? dz[j] : 0.f;
        s1[j] += g;
        s2[j] += g * ((u[j] - mu[j]) * rs[j]);
        o[j] = raw ? dz[j] : a[j] * g;
      }
      if (p.accumulate) {
        float old[CH];
        Chunk<T>::unpack(oq, old);
#pragma unroll
        for (int j = 0; j < CH; ++j) o[j] += old[j];
      }
      *(u32x4*)(yp + (m0 + row) * p.ldy + n) = Chunk<T>::pack(o);
    }
  }
  if (!sums) return;
#pragma unroll
  for (int mask = NCCP; mask < 64; mask <<= 1) {
#pragma unroll
    for (int j = 0; j < CH; ++j) { s1[j] += __shfl_xor(s1[j], mask); s2[j] += __shfl_xor(s2[j], mask); }
  }
  __syncthreads();                                   // every thread is done with the staged tile: its LDS is reused
  float* red = (float*)smem;                         // [4 waves][2][BN]
  const int lane = tid & 63, wave = tid >> 6;
  if (lane < NCCP && cc < NCC) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      red[(wave * 2 + 0) * BN + cc * CH + j] = s1[j];
      red[(wave * 2 + 1) * BN + cc * CH + j] = s2[j];
    }
  }
  __syncthreads();
  float* dst = p.bnb_partial + (long long)(blockIdx.x % (unsigned)p.bnb_slots) * 2 * p.Cout;
  for (int q = tid; q < 2 * BN; q += 256) {
    const int sidx = q / BN, col = q - sidx * BN;
    if (n0 + col < p.Cout) {
      const float t = red[(0 * 2 + sidx) * BN + col] + red[(1 * 2 + sidx) * BN + col] + red[(2 * 2 + sidx) * BN + col] +
                      red[(3 * 2 + sidx) * BN + col];
      atomicAdd(dst + (long long)sidx * p.Cout + n0 + col, t);
    }
  }
}

// ---- epilogue shared by the DMA kernels: bias / dropout in registers, then the tile goes through LDS so that every
// lane writes (and, in accumulate mode, reads) one full 16-byte chunk of a row: 8 lanes cover a 128-byte line.
// BNB: the launch carries the fused BN backward (ConvK::bnb_u != NULL is then a launch-time guarantee: the host picks the
// BNB instantiation for exactly those launches).  `pre_uv` / `pre_ov`: the thread's u / old-gradient chunks when the caller
// already issued them at kernel ENTRY (`preloaded`): they are independent of the GEMM, so the whole K loop hides their
// latency instead of the staging pass of the epilogue (measured round 2: issued late they cost the data-gradient launches
// of the 2D step +2.4 ms).  Kept in a separate instantiation because the 2 x IT x 4 registers they occupy across the K
// loop would otherwise cut the occupancy of every other launch of the tile shape.
template <typename T, int BM, int BN, int WM, int WN, int TM, int TN, int SMEM, bool BNB = false>
__device__ __forceinline__ void igemm_epilogue(const ConvK& p, f32x4 (&acc)[TM][TN], char* smem, long long m0, int n0,
                                               int wm, int wn, int lane, int tid,
                                               u32x4 (&bnb_uv)[BnbGeom<T, BM, BN>::EARLY ? BnbGeom<T, BM, BN>::IT : 1],
                                               u32x4 (&bnb_ov)[BnbGeom<T, BM, BN>::EARLY ? BnbGeom<T, BM, BN>::IT : 1],
                                               bool preloaded) {
  constexpr int CH = Chunk<T>::CH;
  // +16 B: consecutive rows start on different banks; dropped when the padded tile would not fit the operand stages
  // (f32 128x128: 128 * 528 B > 64 KB)
  constexpr int ROWB = BN * (int)sizeof(T) + (BM * (BN * (int)sizeof(T) + 16) <= SMEM ? 16 : 0);
  static_assert(BM * ROWB <= SMEM, "epilogue staging tile must fit the LDS of the operand stages");
  const unsigned dseed = p.drop_seed + (p.drop_seed_dev ? *p.drop_seed_dev : 0u);
  typedef BnbGeom<T, BM, BN> G;
  if constexpr (BNB && G::EARLY) {
    if (!preloaded) bnb_issue_loads<T, BM, BN, G::IT>(p, m0, n0, tid, 0, bnb_uv, bnb_ov);
  }
  __syncthreads();                                   // all MFMA operand reads of the last K tile are done
  // The K loops multiply with the operands SWAPPED (kgroup(b, a, acc)): a lane holds C[m = lane & 15][n = 4 * (lane >> 4)
  // + r] of its 16x16 fragment, i.e. 4 consecutive output channels of one pixel -- one 8- / 16-byte LDS store per
  // fragment instead of four 2- / 4-byte ones.
  const bool has_bias = p.bias != nullptr, drop = p.drop_scale != 0.f, has_epi = p.epi_a != nullptr;
  // this lane's bias / output-affine vectors of its TN column groups: loaded ONCE, unconditionally (clamped channel index),
  // all in flight together.  Round 2's per-fragment "if (n < Cout) v += bias[n]" compiled to a branch + load +
  // s_waitcnt vmcnt(0) per fragment: up to 2 x TM x TN dependent L2 round trips in the epilogue of every biased conv.
  f32x4 bias_v[TN], epa_v[TN], epb_v[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wn * WN + j * 16 + (lane >> 4) * 4;
    const int nc = n < p.Cout ? n : 0;               // Cout is a multiple of the 16-byte chunk: 4 channels are all-or-nothing
    bias_v[j] = has_bias ? *(const f32x4*)(p.bias + nc) : f32x4{0.f, 0.f, 0.f, 0.f};
    epa_v[j] = has_epi ? *(const f32x4*)(p.epi_a + nc) : f32x4{1.f, 1.f, 1.f, 1.f};
    epb_v[j] = has_epi ? *(const f32x4*)(p.epi_b + nc) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row = wm * WM + i * 16 + (lane & 15);
    const long long m = m0 + row;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = wn * WN + j * 16 + (lane >> 4) * 4;
      const int n = n0 + col;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (has_bias) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += bias_v[j][r];
      }
      if (drop) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned h = hdu_hash32((unsigned long long)m * (unsigned)p.Cout + (unsigned)(n + r), dseed);
          v[r] = h < p.drop_thresh ? v[r] * p.drop_scale : 0.f;
        }
      }
      if (has_epi) {                                 // the BN(+Scale)(+ReLU) that follows this conv (stored statistics)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = epa_v[j][r] * v[r] + epb_v[j][r];
          if (p.epi_relu) v[r] = v[r] > 0.f ? v[r] : 0.f;
        }
      }
      Chunk<T>::store4((T*)(smem + row * ROWB) + col, v);
    }
  }
  __syncthreads();
  HDU_TP(7);                                         // (timeline builds: the tile is staged)
  if constexpr (BNB) {                               // data gradient with the consumer BN's backward fused in
    epilogue_bn_backward<T, BM, BN, ROWB>(p, smem, m0, n0, tid, bnb_uv, bnb_ov);
    return;
  }
  T* __restrict__ yp = (T*)p.y;
  constexpr int NCC = BN / CH;                       // 16-byte chunks per tile row
  constexpr int NIT = (BM * NCC + 255) / 256;
  if (p.accumulate) {
    // read-modify-write: ALL of this thread's old chunks are requested before the first one is used (the accumulators
    // are dead, their registers hold the loads) -- one memory round trip per tile instead of one per chunk
    u32x4 old[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int q = tid + it * 256;
      const int row = q / NCC, cc = q % NCC;
      const long long m = m0 + row;
      const int n = n0 + cc * CH;
      // unconditional (see bnb_issue_loads): lanes without a chunk re-read element 0 and ignore it below
      const bool ok = q < BM * NCC && m < p.M && n < p.Cout;
      old[it] = *(const u32x4*)(yp + (ok ? m * p.ldy + n : 0));
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int q = tid + it * 256;
      const int row = q / NCC, cc = q % NCC;
      const long long m = m0 + row;
      const int n = n0 + cc * CH;
      if (q >= BM * NCC || m >= p.M || n >= p.Cout) continue;
      float f[CH], g[CH];
      Chunk<T>::unpack(*(const u32x4*)(smem + row * ROWB + cc * 16), f);
      Chunk<T>::unpack(old[it], g);
#pragma unroll
      for (int jj = 0; jj < CH; ++jj) f[jj] += g[jj];
      *(u32x4*)(yp + m * p.ldy + n) = Chunk<T>::pack(f);
    }
  } else {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int q = tid + it * 256;
      const int row = q / NCC, cc = q % NCC;
      const long long m = m0 + row;
      const int n = n0 + cc * CH;
      if (q >= BM * NCC || m >= p.M || n >= p.Cout) continue;      // Cout is a multiple of CH: chunks are all-or-nothing
      *(u32x4*)(yp + m * p.ldy + n) = *(const u32x4*)(smem + row * ROWB + cc * 16);
    }
  }
  if (p.stats_partial)
    epilogue_stats<T, BM, BN, ROWB>(p, smem, n0, tid, blockIdx.x, [&](int row) { return m0 + row < p.M; });
}

// =====================================================================================
// DMA form of the implicit GEMM: used whenever the operand gather needs no arithmetic (no BN/ReLU prologue, no
// skip add) -- i.e. for materialised inputs, for every data gradient and for all filter tiles.  Each lane issues
// global_load_lds_dwordx4 straight into the swizzled LDS tile (no VGPR staging, no ds_write, no VALU on data);
// padding / tails read a 16-byte page of zeros.  The LDS image is lane-linear per wave instruction, so the XOR
// swizzle is applied by permuting which logical k-chunk each lane fetches.
__device__ __attribute__((aligned(16))) unsigned hdu_zero_page[16];
// Developer instrumentation (tools/timeline_probe.py builds its own library with -DHDU_TIMELINE; never in libhdu.so):
// lane 0 of every workgroup stamps the shader clock at a few points of the implicit-GEMM kernels, plus the constant
// 100 MHz clock at entry / exit so that workgroups of different XCDs share one time axis.


// ---- BN(+Scale)+ReLU of the PRODUCER applied to the A operand of a POINTWISE conv on its way from LDS to the MFMA (PRO).
// The dense-block bottleneck reads relu(a[c] * slab[m][c] + b[c]) for ALL channels written so far (denseunet.py:245-248,
// denseunet3d.py:31-38): materialising that operand costs a full read + write of an O(L^2) tensor per layer (rounds 1-3:
// 3.2 GB per 2D step).  Here the raw slab is DMA'd as it is; the per-channel a / b (the whole contraction range: <= 18 KB)
// are DMA'd ONCE into an LDS table ahead of the first operand tile, and a lane transforms its 16-byte fragment (CH
// consecutive channels of one pixel) in registers between ds_read and MFMA: 2 table reads + ~3 VALU per element, against
// the 6-12 MFMAs the fragment feeds.  Rows past M and channels past Cin arrive as zeros and leave as relu(b) / 0 (the table
// is zero-filled past Cin): finite values that are multiplied by zero filter columns or never stored.
// Table capacity PROC (channels) is a template parameter of the kernels: 2304 covers the widest contraction of the path
// (2D block 5: 2160 channels, 18 KB of LDS), 1024 (8 KB) keeps two workgroups of the widest tiles on a CU for the 3D nets
// and the early 2D blocks.  The host picks the smallest capacity >= Cin.
constexpr int HDU_PRO_CMAX = 2304;
constexpr int HDU_PRO_CSMALL = 1024;

template <typename T>
__device__ __forceinline__ u32x4 pro_apply(u32x4 v, const float* __restrict__ ta, const float* __restrict__ tb, float lo) {
  constexpr int CH = Chunk<T>::CH;
  float f[CH];
  Chunk<T>::unpack(v, f);
#pragma unroll
  for (int j = 0; j < CH; j += 4) {
    const f32x4 a4 = *(const f32x4*)(ta + j), b4 = *(const f32x4*)(tb + j);
#pragma unroll
    for (int r = 0; r < 4; ++r) f[j + r] = fmaxf(a4[r] * f[j + r] + b4[r], lo);
  }
  return Chunk<T>::pack(f);
}

// fills the LDS table [a: HDU_PRO_CMAX floats][b: HDU_PRO_CMAX floats] with async buffer DMAs (1 KiB = 256 channels per
// wave instruction; out-of-range lanes write zeros).  Issued BEFORE the first operand tile: older than every operand DMA, so
// the K loops' vmcnt waits cover it.  `cin64` = Cin rounded up to the K step.
template <int PROC>
__device__ __forceinline__ void pro_table_issue(const ConvK& p, char* tab, int wave, int lane) {
  const hdu_bufsrd asrd = hdu_make_srd(p.pro_a, (unsigned)p.Cin * 4u);
  const hdu_bufsrd bsrd = hdu_make_srd(p.pro_b, (unsigned)p.Cin * 4u);
  const int nch = (p.Cin + 255) >> 8;                  // 256-channel pieces (the tail of the last one reads zeros)
  for (int q = wave; q < 2 * nch; q += 4) {            // wave-uniform
    const bool isb = q >= nch;
    const int c = isb ? q - nch : q;
    const unsigned off = (unsigned)(c * 256 + lane * 4) * 4u;
    hdu_bufload_lds16(isb ? bsrd : asrd, off, tab + (isb ? PROC * 4 : 0) + c * 1024);
  }
}

template <bool SPLIT, typename T, int BM, int BN, int WAVES_M, int WAVES_N, bool FAST, bool BNB, int PROC>
__device__ __forceinline__ void conv_igemm_dma_body(const ConvK& p, char* smem) {
  constexpr bool PRO = PROC > 0;
  constexpr int CH = Chunk<T>::CH;
  constexpr int BK = 8 * CH;
  constexpr int A_IT = BM / 32;
  constexpr int B_IT = (BN + 31) / 32;
  constexpr int WM = BM / WAVES_M;
  constexpr int WN = BN / WAVES_N;
  constexpr int TM = WM / 16;
  constexpr int TN = WN / 16;
  constexpr int STAGE = (BM + BN) * 128;
  static_assert(WAVES_M * WAVES_N == 4, "4 waves");
  static_assert(!(PRO && BNB), "the operand prologue belongs to forward launches, the fused BN backward to data gradients");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
#ifdef HDU_EMU
  const int wave = tid >> 6;
#else
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#endif
  if constexpr (PRO) pro_table_issue<PROC>(p, smem + 2 * STAGE, wave, lane);
  const float* pro_ta = (const float*)(smem + 2 * STAGE);
  const float* pro_tb = pro_ta + PROC;
  const float pro_lo = p.pro_relu ? 0.f : -__builtin_huge_valf();
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;
  const int r0 = tid >> 3;
  const int kcl = (tid & 7) ^ (r0 & 7);   // logical chunk this lane fetches (it lands at physical chunk tid&7)
  const long long m0 = (long long)((p.xcd_swizzle & 1) ? xcd_tile_index(blockIdx.x, gridDim.x) : blockIdx.x) * BM;
  const int n0 = blockIdx.y * BN;
  HDU_TP(0);
  const T* __restrict__ xp = (const T*)p.x;
  const T* __restrict__ wp = (const T*)p.w;
  const char* zero = (const char*)hdu_zero_page;
  const bool ups = (p.ud | p.uh | p.uw) != 0;

  const bool pointwise = p.KD * p.KH * p.KW == 1 && p.sd == 1 && p.sh == 1 && p.sw == 1 && (p.pd | p.ph | p.pw) == 0 &&
                         !(p.debug_flags & 8);
  // per-row state.  FAST (no up-sampling, <= 32 taps, tensor < 2^31 elements): a tap-validity bitmask and an
  // element offset per row are computed ONCE, so a DMA in the K loop costs a shift/and, one add and the pointer add.
  int rn[A_IT], rid[A_IT], rih[A_IT], riw[A_IT], rpix[A_IT];
  unsigned rmask[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i)     // M < 2^31 (checked on the host)
    hdu_row_state<FAST>(p, (unsigned)(m0 + r0 + i * 32), pointwise, rn[i], rid[i], rih[i], riw[i], rpix[i], rmask[i]);
  int k = kcl * CH;
  int c, kd, kh, kw, tap_i;
  hdu_k_state(p, k, c, kd, kh, kw, tap_i);
  // filter rows of this lane
  // operands arrive through buffer resources (hdu_platform.h): 32-bit byte offsets, out-of-range = zeros
  const hdu_bufsrd xsrd = hdu_make_srd(xp, p.x_bytes);
  const hdu_bufsrd wsrd = hdu_make_srd(wp, p.w_bytes);
  const bool small_x = p.x_bytes != 0u;
  int wrow[B_IT];                    // element offset of this lane's filter row, -1 = no such row
#pragma unroll
  for (int j = 0; j < B_IT; ++j) {
    const int col = n0 + r0 + j * 32;
    wrow[j] = (r0 + j * 32 < BN && col < p.Cout) ? col * p.Ktot : -1;
  }

  auto issue_tile = [&](int buf) {
    char* As = smem + buf * STAGE;
    char* Bs = As + BM * 128;
    const bool kvalid = kd < p.KD;
    const int tapoff = (kd * p.He + kh) * p.We + kw;
    if (FAST) {
      const int toff = tapoff * (int)p.ldx + c;            // element offset of this lane's (tap, channel chunk)
#pragma unroll
      for (int i = 0; i < A_IT; ++i) {
        const bool ok = kvalid && ((rmask[i] >> tap_i) & 1u);
        hdu_bufload_lds16(xsrd, ok ? (unsigned)(rpix[i] + toff) * (unsigned)sizeof(T) : HDU_OOB, As + (i * 32 + wave * 8) * 128);
      }
    } else {
#pragma unroll
      for (int i = 0; i < A_IT; ++i) {
        const int id = rid[i] + kd, ih = rih[i] + kh, iw = riw[i] + kw;
        const bool ok = kvalid && (unsigned)id < (unsigned)p.De && (unsigned)ih < (unsigned)p.He &&
                        (unsigned)iw < (unsigned)p.We;
        const int src = ups ? ((rn[i] * p.Di + (id >> p.ud)) * p.Hi + (ih >> p.uh)) * p.Wi + (iw >> p.uw)
                            : rpix[i] + tapoff;
        if (small_x) {       // the stored tensor fits a 32-bit byte offset: buffer form (wave-uniform branch)
          hdu_bufload_lds16(xsrd, ok ? ((unsigned)src * (unsigned)p.ldx + (unsigned)c) * (unsigned)sizeof(T) : HDU_OOB,
                            As + (i * 32 + wave * 8) * 128);
        } else {
          const char* g = ok ? (const char*)(xp + (long long)src * p.ldx + c) : zero;
          hdu_glds16(g, As + (i * 32 + wave * 8) * 128);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < B_IT; ++j) {
      if (j * 32 + wave * 8 < BN) {   // wave-uniform
        hdu_bufload_lds16(wsrd, (wrow[j] >= 0 && k < p.Ktot) ? (unsigned)(wrow[j] + k) * (unsigned)sizeof(T) : HDU_OOB,
                          Bs + (j * 32 + wave * 8) * 128);
      }
    }
  };

  auto advance = [&]() {
    k += BK;
    c += BK;
    while (c >= p.Cin) {
      c -= p.Cin;
      ++tap_i;
      if (++kw == p.KW) {
        kw = 0;
        if (++kh == p.KH) {
          kh = 0;
          ++kd;
        }
      }
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (p.Ktot + BK - 1) / BK;
  // fused BN backward: this thread's u / old-gradient chunks are requested now, ahead of every operand DMA
  typedef BnbGeom<T, BM, BN> BG;
  u32x4 bnb_uv[BG::EARLY ? BG::IT : 1], bnb_ov[BG::EARLY ? BG::IT : 1];
  const bool bnb_pre = BNB && BG::EARLY && !(p.debug_flags & 32);
  if constexpr (BNB && BG::EARLY) {
    if (bnb_pre) {
      bnb_issue_loads<T, BM, BN, BG::IT>(p, m0, n0, tid, 0, bnb_uv, bnb_ov);
      HDU_SCHED_BARRIER();
    }
  }
  HDU_TP(1);
  issue_tile(0);
  HDU_TP(2);
  __syncthreads();
  HDU_TP(3);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) {
      advance();
      if (!(p.debug_flags & 1)) issue_tile(buf ^ 1);     // debug: measure the loop without operand traffic
    }
    if (!(p.debug_flags & 2)) {                           // debug: measure the loop without MFMA / LDS reads
      const char* As = smem + buf * STAGE;
      const char* Bs = As + BM * 128;
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        u32x4 af[TM], bf[TN];
        const int chunk = kg * 4 + (lane >> 4);
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = *(const u32x4*)(As + lds_chunk_off(wm * WM + i * 16 + (lane & 15), chunk));
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = *(const u32x4*)(Bs + lds_chunk_off(wn * WN + j * 16 + (lane & 15), chunk));
        if constexpr (PRO) {                                 // pointwise: GEMM column k IS the input channel
          const int cb = kt * BK + chunk * CH;
#pragma unroll
          for (int i = 0; i < TM; ++i) af[i] = pro_apply<T>(af[i], pro_ta + cb, pro_tb + cb, pro_lo);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = Mma<T>::template kgroup<SPLIT>(bf[j], af[i], acc[i][j]);   // transposed tile: see igemm_epilogue
      }
    }
    __syncthreads();
  }

  HDU_TP(4);
  HDU_TP(5);
  igemm_epilogue<T, BM, BN, WM, WN, TM, TN, 2 * STAGE, BNB>(p, acc, smem, m0, n0, wm, wn, lane, tid, bnb_uv, bnb_ov, bnb_pre);
  HDU_TP(6);
}

// the float32 instantiations carry both contraction forms (ConvK::f32_split, Mma<float>): one uniform branch at entry
template <typename T, int BM, int BN, int WAVES_M, int WAVES_N, bool FAST, bool BNB = false, int PROC = 0>
__global__ __launch_bounds__(256) void conv_igemm_dma_kernel(ConvK p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * (BM + BN) * 128 + 2 * PROC * 4];
  if constexpr (sizeof(T) == 4) {
    if (p.f32_split) { conv_igemm_dma_body<true, T, BM, BN, WAVES_M, WAVES_N, FAST, BNB, PROC>(p, smem); return; }
  }
  conv_igemm_dma_body<false, T, BM, BN, WAVES_M, WAVES_N, FAST, BNB, PROC>(p, smem);
}

// NS-stage ring variant: tiles t+1 .. t+NS-1 stay in flight while tile t is multiplied.  Per iteration: counted
// vmcnt (this wave's DMAs of tile t have landed) -> ONE raw barrier (everyone's have; everyone finished reading the
// slot about to be refilled) -> issue tile t+NS-1 -> MFMAs on tile t.  Every wave issues exactly A_IT + B_IT DMAs
// per tile (invalid rows read out of range = zeros, or the zero page) so the vmcnt immediate is uniform.  Used for small grids (< 1
// workgroup per CU), where latency rather than occupancy limits the K loop and one workgroup may take the LDS.
// split-K meeting point of the ring kernel (hdu_platform.h: hdu_store_wt16 / hdu_acquire_agent).  Every split stores its
// accumulator fragments lane-linear ([wave][fragment][lane] x 16 B: one coalesced 1 KiB store per fragment and wave),
// drains, and takes a ticket; the last arriver sums all splits' fragments (same lane mapping, plain 16-byte loads after
// ONE agent-scope acquire) and returns true: it alone runs the ordinary epilogue.
template <int TM, int TN>
__device__ __forceinline__ bool splitk_combine(const ConvK& p, f32x4 (&acc)[TM][TN], char* smem, unsigned tile, int z, int S,
                                               int wave, int lane, int tid) {
  constexpr int FR = TM * TN;
  constexpr size_t SPLIT_FLOATS = (size_t)4 * FR * 64 * 4;
  float* base = p.sk_ws + (size_t)tile * (size_t)S * SPLIT_FLOATS;
  float* mine = base + (size_t)z * SPLIT_FLOATS + ((size_t)wave * FR) * 256 + lane * 4;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) hdu_store_wt16(mine + (i * TN + j) * 256, acc[i][j]);
  HDU_WAIT_STORES();                                  // every storing wave drains its write-through stores ...
  __syncthreads();                                    // ... before ONE lane announces the workgroup's arrival
  int* flag = (int*)smem;                             // the operand stages are dead: all MFMA reads are behind the barrier
  if (tid == 0) *flag = hdu_ticket(p.sk_cnt + tile) == (unsigned)(S - 1) ? 1 : 0;
  __syncthreads();
  if (*flag == 0) return false;
  if (tid == 0) hdu_acquire_agent();
  __syncthreads();
  // fixed summation order 0..S-1 whichever split arrives last (its own fragments are re-read too): the result does not
  // depend on the arrival order, so a layer is reproducible run to run
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < S; ++s) {
    const float* o = base + (size_t)s * SPLIT_FLOATS + ((size_t)wave * FR) * 256 + lane * 4;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const f32x4 v = *(const f32x4*)(o + (i * TN + j) * 256);
        acc[i][j] += v;
      }
  }
  if (tid == 0) hdu_store_agent_u32(p.sk_cnt + tile, 0u);     // the counter is zero again for the next launch
  return true;
}

// counted vector-memory wait with a compile-time count (an "i" operand prints as the literal s_waitcnt needs; vmcnt is
// 6 bits on gfx950)
template <int N> __device__ __forceinline__ void hdu_wait_vmcnt_n() {
  static_assert(N >= 0 && N < 64, "vmcnt immediate");
#ifndef HDU_EMU
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
#endif
}

template <bool SPLIT, typename T, int BM, int BN, int WAVES_M, int WAVES_N, int NS, bool FAST, bool BNB, int PROC>
__device__ __forceinline__ void conv_igemm_ring_body(const ConvK& p, char* smem) {
  constexpr bool PRO = PROC > 0;
  constexpr int CH = Chunk<T>::CH;
  constexpr int BK = 8 * CH;
  constexpr int A_IT = BM / 32;
  constexpr int B_IT = (BN + 31) / 32;
  constexpr int BNP = B_IT * 32;
  constexpr int WM = BM / WAVES_M;
  constexpr int WN = BN / WAVES_N;
  constexpr int TM = WM / 16;
  constexpr int TN = WN / 16;
  constexpr int STAGE = (BM + BNP) * 128;
  constexpr int L = A_IT + B_IT;
  static_assert(WAVES_M * WAVES_N == 4, "4 waves");
  static_assert(!(PRO && BNB), "the operand prologue belongs to forward launches, the fused BN backward to data gradients");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
#ifdef HDU_EMU
  const int wave = tid >> 6;
#else
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#endif
  // (the table DMAs are older than every operand DMA: the counted vmcnt waits of the ring still mean what they say)
  if constexpr (PRO) pro_table_issue<PROC>(p, smem + NS * STAGE, wave, lane);
  const float* pro_ta = (const float*)(smem + NS * STAGE);
  const float* pro_tb = pro_ta + PROC;
  const float pro_lo = p.pro_relu ? 0.f : -__builtin_huge_valf();
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;
  const int r0 = tid >> 3;
  const int kcl = (tid & 7) ^ (r0 & 7);
  const long long m0 = (long long)((p.xcd_swizzle & 1) ? xcd_tile_index(blockIdx.x, gridDim.x) : blockIdx.x) * BM;
  const int n0 = blockIdx.y * BN;
  HDU_TP(0);
  const T* __restrict__ xp = (const T*)p.x;
  const T* __restrict__ wp = (const T*)p.w;
  const char* zero = (const char*)hdu_zero_page;
  const bool ups = (p.ud | p.uh | p.uw) != 0;

  const bool pointwise = p.KD * p.KH * p.KW == 1 && p.sd == 1 && p.sh == 1 && p.sw == 1 && (p.pd | p.ph | p.pw) == 0 &&
                         !(p.debug_flags & 8);
  // per-row state.  FAST (no up-sampling, <= 32 taps, tensor < 2^31 elements): a tap-validity bitmask and an
  // element offset per row are computed ONCE, so a DMA in the K loop costs a shift/and, one add and the pointer add.
  int rn[A_IT], rid[A_IT], rih[A_IT], riw[A_IT], rpix[A_IT];
  unsigned rmask[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i)     // M < 2^31 (checked on the host)
    hdu_row_state<FAST>(p, (unsigned)(m0 + r0 + i * 32), pointwise, rn[i], rid[i], rih[i], riw[i], rpix[i], rmask[i]);
  // split-K: gridDim.z workgroups share this output tile, each takes a contiguous range of K steps
  const int nk_all = (p.Ktot + BK - 1) / BK;
  const int nsplit = (int)gridDim.z, split = (int)blockIdx.z;
  // split s takes K steps [nk * s / S, nk * (s + 1) / S)
  const int kt_begin = nsplit > 1 ? (int)hdu_fastdiv((unsigned)(nk_all * split), p.sk_div_mul, p.sk_div_shr) : 0;
  const int kt_end = nsplit > 1 ? (int)hdu_fastdiv((unsigned)(nk_all * (split + 1)), p.sk_div_mul, p.sk_div_shr) : nk_all;
  int k = kt_begin * BK + kcl * CH;
  int c, kd, kh, kw, tap_i;
  hdu_k_state(p, k, c, kd, kh, kw, tap_i);
  // operands arrive through buffer resources (hdu_platform.h): 32-bit byte offsets, out-of-range = zeros
  const hdu_bufsrd xsrd = hdu_make_srd(xp, p.x_bytes);
  const hdu_bufsrd wsrd = hdu_make_srd(wp, p.w_bytes);
  const bool small_x = p.x_bytes != 0u;
  int wrow[B_IT];                    // element offset of this lane's filter row, -1 = no such row
#pragma unroll
  for (int j = 0; j < B_IT; ++j) {
    const int col = n0 + r0 + j * 32;
    wrow[j] = (r0 + j * 32 < BN && col < p.Cout) ? col * p.Ktot : -1;
  }

  auto issue_tile = [&](int slot) {
    char* As = smem + slot * STAGE;
    char* Bs = As + BM * 128;
    const bool kvalid = kd < p.KD;
    const int tapoff = (kd * p.He + kh) * p.We + kw;
    if (FAST) {
      const int toff = tapoff * (int)p.ldx + c;            // element offset of this lane's (tap, channel chunk)
#pragma unroll
      for (int i = 0; i < A_IT; ++i) {
        const bool ok = kvalid && ((rmask[i] >> tap_i) & 1u);
        hdu_bufload_lds16(xsrd, ok ? (unsigned)(rpix[i] + toff) * (unsigned)sizeof(T) : HDU_OOB, As + (i * 32 + wave * 8) * 128);
      }
    } else {
#pragma unroll
      for (int i = 0; i < A_IT; ++i) {
        const int id = rid[i] + kd, ih = rih[i] + kh, iw = riw[i] + kw;
        const bool ok = kvalid && (unsigned)id < (unsigned)p.De && (unsigned)ih < (unsigned)p.He &&
                        (unsigned)iw < (unsigned)p.We;
        const int src = ups ? ((rn[i] * p.Di + (id >> p.ud)) * p.Hi + (ih >> p.uh)) * p.Wi + (iw >> p.uw)
                            : rpix[i] + tapoff;
        if (small_x) {       // the stored tensor fits a 32-bit byte offset: buffer form (wave-uniform branch)
          hdu_bufload_lds16(xsrd, ok ? ((unsigned)src * (unsigned)p.ldx + (unsigned)c) * (unsigned)sizeof(T) : HDU_OOB,
                            As + (i * 32 + wave * 8) * 128);
        } else {
          const char* g = ok ? (const char*)(xp + (long long)src * p.ldx + c) : zero;
          hdu_glds16(g, As + (i * 32 + wave * 8) * 128);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < B_IT; ++j) {
      hdu_bufload_lds16(wsrd, (wrow[j] >= 0 && k < p.Ktot) ? (unsigned)(wrow[j] + k) * (unsigned)sizeof(T) : HDU_OOB,
                        Bs + (j * 32 + wave * 8) * 128);
    }
    // advance this lane's k state to the next tile
    k += BK;
    c += BK;
    while (c >= p.Cin) {
      c -= p.Cin;
      ++tap_i;
      if (++kw == p.KW) {
        kw = 0;
        if (++kh == p.KH) {
          kh = 0;
          ++kd;
        }
      }
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = kt_end - kt_begin;
  // fused BN backward (unsplit launches only: a split's epilogue runs in whichever workgroup arrives last): the u /
  // old-gradient chunks are requested ahead of every operand DMA -- older than all of them, so the ring's counted vmcnt
  // waits still mean what they say
  typedef BnbGeom<T, BM, BN> BG;
  u32x4 bnb_uv[BG::EARLY ? BG::IT : 1], bnb_ov[BG::EARLY ? BG::IT : 1];
  const bool bnb_pre = BNB && BG::EARLY && nsplit == 1 && !(p.debug_flags & 32);
  if constexpr (BNB && BG::EARLY) {
    if (bnb_pre) {
      bnb_issue_loads<T, BM, BN, BG::IT>(p, m0, n0, tid, 0, bnb_uv, bnb_ov);
      HDU_SCHED_BARRIER();
    }
  }
  HDU_TP(1);
#pragma unroll
  for (int pre = 0; pre < NS - 1; ++pre)
    if (pre < nk) issue_tile(pre);
  HDU_TP(2);
  int slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // tiles issued beyond kt: min(NS-2, nk-1-kt) may stay in flight
    const int ahead = nk - 1 - kt;
    if (ahead >= NS - 2) hdu_wait_vmcnt_n<(NS - 2) * L>();
    else if (NS > 3 && ahead == 1) hdu_wait_vmcnt_n<L>();
    else if (NS > 4 && ahead == 2) hdu_wait_vmcnt_n<2 * L>();
    else if (NS > 5 && ahead == 3) hdu_wait_vmcnt_n<3 * L>();
    else hdu_wait_vmcnt_n<0>();
    HDU_RAW_BARRIER();
#ifdef HDU_TIMELINE
    if (kt == 0) HDU_TP(3);
#endif
    if (kt + NS - 1 < nk) issue_tile(slot == 0 ? NS - 1 : slot - 1);   // slot (kt+NS-1) % NS
    {
      const char* As = smem + slot * STAGE;
      const char* Bs = As + BM * 128;
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        u32x4 af[TM], bf[TN];
        const int chunk = kg * 4 + (lane >> 4);
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = *(const u32x4*)(As + lds_chunk_off(wm * WM + i * 16 + (lane & 15), chunk));
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = *(const u32x4*)(Bs + lds_chunk_off(wn * WN + j * 16 + (lane & 15), chunk));
        if constexpr (PRO) {                                 // pointwise: GEMM column k IS the input channel
          const int cb = (kt_begin + kt) * BK + chunk * CH;
#pragma unroll
          for (int i = 0; i < TM; ++i) af[i] = pro_apply<T>(af[i], pro_ta + cb, pro_tb + cb, pro_lo);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = Mma<T>::template kgroup<SPLIT>(bf[j], af[i], acc[i][j]);   // transposed tile: see igemm_epilogue
      }
    }
    slot = slot == NS - 1 ? 0 : slot + 1;
  }

  HDU_TP(4);
  if (nsplit > 1) {
    HDU_WAIT_VMCNT(0);
    if (!splitk_combine<TM, TN>(p, acc, smem, blockIdx.y * gridDim.x + blockIdx.x, split, nsplit, wave, lane, tid)) {
      HDU_TP(5);
      return;
    }
  }
  HDU_TP(5);
  igemm_epilogue<T, BM, BN, WM, WN, TM, TN, NS * STAGE, BNB>(p, acc, smem, m0, n0, wm, wn, lane, tid, bnb_uv, bnb_ov, bnb_pre);
  HDU_TP(6);
}

// the float32 instantiations carry both contraction forms (ConvK::f32_split, Mma<float>): one uniform branch at entry
template <typename T, int BM, int BN, int WAVES_M, int WAVES_N, int NS, bool FAST, bool BNB = false, int PROC = 0>
__global__ __launch_bounds__(256) void conv_igemm_ring_kernel(ConvK p) {
  __shared__ __attribute__((aligned(16))) char smem[NS * (BM + (BN + 31) / 32 * 32) * 128 + 2 * PROC * 4];
  if constexpr (sizeof(T) == 4) {
    if (p.f32_split) { conv_igemm_ring_body<true, T, BM, BN, WAVES_M, WAVES_N, NS, FAST, BNB, PROC>(p, smem); return; }
  }
  conv_igemm_ring_body<false, T, BM, BN, WAVES_M, WAVES_N, NS, FAST, BNB, PROC>(p, smem);
}

// =====================================================================================
// Persistent form of the implicit GEMM for LARGE grids (round 4).
// The two-stage kernel above keeps ONE 28 KB operand stage in flight per workgroup and pays row decode, first-tile latency
// and the epilogue per 128 x BN tile, hidden only by the second workgroup of the CU (measured round 2: the K loop is half of
// a workgroup's life; 23 B/clk/CU of the ~50 the L2 -> LDS path delivers; MFMA busy 16 %).  Here ONE 512-thread workgroup
// per CU owns the CU's LDS and walks a list of 256 x BN tiles:
//   * a 3-slot ring of (256 + BN) x 128 B stages that runs ACROSS tile boundaries: while the last K steps of tile t are
//     multiplied the first stages of tile t+1 are already in flight (row decode of t+1 included), two stages = ~90 KB in
//     flight per CU, counted vmcnt + one raw barrier per K step;
//   * 8 waves (2 per SIMD: one wave's MFMAs overlap the other's DMA issue / epilogue), each 32 rows x BN columns;
//   * the epilogue leaves the LDS alone: a lane holds 4 consecutive output channels of one pixel (operands swapped in the
//     MFMA), so bias / dropout / output affine / accumulate / the 8- or 16-byte store happen in registers, the statistics as
//     DPP row sums + one atomic instruction per 16-column group -- no barrier, it overlaps the next tile's DMAs;
//   * 256 rows per filter tile: 21 % fewer operand bytes per FLOP than 128 x 96.
// MEASURED (MI355X, profiles/r04_experiment_persistent_gemm.txt): correct, and 10-20 % SLOWER per launch than the two-stage
// kernel on every one of the 25 large-grid launches of the 2D step (2D 17.5 -> 17.9 ms with 8 lock-stepped waves, 17.7 with the
// two waves of a SIMD in opposite phase order; a 4-wave form with 64 x BN outputs per wave: 22 ms).  Both forms move ~23 B/clk/CU
// through the L2 -> LDS path whatever the pipeline depth: with ~0.65 KiB of LDS fragment reads per MFMA on top of the DMA
// writes the LDS itself is ~60 % busy, and two independent 4-wave workgroups interleave their DMA / MFMA / epilogue phases
// better than 8 waves behind one barrier per K step.  OFF by default (HDU_TUNE_PERS = 1 / HDU_PERS=1 turns it on); kept as a
// tested, measured option.
// m-tiles are dealt round-robin to the workgroups; a workgroup visits all n-tiles of an m-tile back to back (the A rows come
// from its XCD's L2 the second time).  FAST addressing only (no up-sampling, <= 32 taps, tensor < 4 GiB), no fused BN
// backward; the BN(+Scale)+ReLU operand prologue of a pointwise conv (PROC > 0) as in the kernels above.
template <typename T, int BN, int PROC = 0, int NW = 8>
__global__ __launch_bounds__(NW * 64) void conv_igemm_pers_kernel(ConvK p, int tiles_m, int tiles_n) {
  constexpr int CH = Chunk<T>::CH;
  constexpr int BK = 8 * CH;
  constexpr int BM = 256, NS = 3;
  constexpr int RP = NW * 8;                      // rows one pass of the workgroup's DMA instructions covers
  constexpr int A_IT = BM / RP;
  constexpr int B_IT = (BN + RP - 1) / RP;
  constexpr int WM = BM / NW, TM = WM / 16, TN = BN / 16;
  constexpr int STAGE = (BM + BN) * 128;
  constexpr bool PRO = PROC > 0;
  static_assert(BN % 16 == 0 && NS * STAGE + 8 * PROC <= 160 * 1024, "tile / LDS");
  __shared__ __attribute__((aligned(16))) char smem[NS * STAGE + 8 * PROC];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
#ifdef HDU_EMU
  const int wave = tid >> 6;
#else
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#endif
  if constexpr (PRO) {     // per-channel a / b of the whole contraction range: once per workgroup, older than every operand DMA
    const hdu_bufsrd asrd = hdu_make_srd(p.pro_a, (unsigned)p.Cin * 4u);
    const hdu_bufsrd bsrd = hdu_make_srd(p.pro_b, (unsigned)p.Cin * 4u);
    const int nch = (p.Cin + 255) >> 8;
    for (int q = wave; q < 2 * nch; q += NW) {
      const bool isb = q >= nch;
      const int cq = isb ? q - nch : q;
      hdu_bufload_lds16(isb ? bsrd : asrd, (unsigned)(cq * 256 + lane * 4) * 4u, smem + NS * STAGE + (isb ? PROC * 4 : 0) + cq * 1024);
    }
  }
  const float* pro_ta = (const float*)(smem + NS * STAGE);
  const float* pro_tb = pro_ta + PROC;
  const float pro_lo = p.pro_relu ? 0.f : -__builtin_huge_valf();
  const int r0 = tid >> 3;                       // 0..RP-1: this lane stages rows r0 + RP * i
  const int kcl = (tid & 7) ^ (r0 & 7);          // logical 16-byte chunk it fetches (lands at physical chunk tid & 7)
  const T* __restrict__ xp = (const T*)p.x;
  const T* __restrict__ wp = (const T*)p.w;
  const hdu_bufsrd xsrd = hdu_make_srd(xp, p.x_bytes);
  const hdu_bufsrd wsrd = hdu_make_srd(wp, p.w_bytes);
  const bool pointwise = p.KD * p.KH * p.KW == 1 && p.sd == 1 && p.sh == 1 && p.sw == 1 && (p.pd | p.ph | p.pw) == 0;
  const int nk = (p.Ktot + BK - 1) / BK;
  // filter rows this wave's DMA instructions cover: instruction j holds rows j * RP + wave * 8 .. + 7 (wave-uniform count)
  int nb_w = 0;
#pragma unroll
  for (int j = 0; j < B_IT; ++j) nb_w += (j * RP + wave * 8 < BN) ? 1 : 0;

  // work items = (m-tile, n-tile) pairs.  Enough m-tiles for every workgroup: a workgroup takes m-tiles b, b + G, ... and
  // visits all n-tiles of each back to back (the A rows come from its XCD's L2 the second time); fewer: the pairs are dealt
  // round-robin.  `nitems` = pairs of this workgroup.
  const int G = (int)gridDim.x, bx = (int)blockIdx.x;
  const bool by_mtile = tiles_m >= G;
  const int nitems = by_mtile ? ((tiles_m - bx + G - 1) / G) * tiles_n : (tiles_m * tiles_n - bx + G - 1) / G;
  auto item_pos = [&](int it, int& mt, int& nt) {
    if (it >= nitems) { mt = tiles_m; nt = 0; return; }       // past the list: nothing valid
    if (by_mtile) {
      const int q = it / tiles_n;
      mt = bx + q * G;
      nt = it - q * tiles_n;
    } else {
      const int w = bx + it * G;
      mt = w / tiles_n;
      nt = w - mt * tiles_n;
    }
  };
  // ---- LOAD side: position (item, K step) of the next stage to request
  int l_it = 0, l_mt, l_nt, l_kt = 0;
  item_pos(0, l_mt, l_nt);
  int rpix[A_IT];
  unsigned rmask[A_IT];
  int wrow[B_IT];
  int k, c, kd, kh, kw, tap_i;
  auto tile_state = [&]() {
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      int rn, rid, rih, riw;
      if (l_mt < tiles_m) {
        hdu_row_state<true>(p, (unsigned)(l_mt * BM + r0 + i * RP), pointwise, rn, rid, rih, riw, rpix[i], rmask[i]);
      } else {
        rpix[i] = 0;
        rmask[i] = 0u;
      }
    }
  };
  auto n_state = [&]() {
#pragma unroll
    for (int j = 0; j < B_IT; ++j) {
      const int row = r0 + j * RP;
      const int col = l_nt * BN + row;
      wrow[j] = (row < BN && col < p.Cout && l_mt < tiles_m) ? col * p.Ktot : -1;
    }
  };
  auto k_reset = [&]() {
    k = kcl * CH;
    hdu_k_state(p, k, c, kd, kh, kw, tap_i);
  };
  // every call issues exactly A_IT + nb_w DMA instructions per wave (a position past the tile list reads out of range =
  // zeros into a slot nobody multiplies), so the counted waits below are uniform
  auto issue = [&](int slot) {
    char* As = smem + slot * STAGE;
    char* Bs = As + BM * 128;
    const bool kvalid = kd < p.KD;
    const int toff = ((kd * p.He + kh) * p.We + kw) * (int)p.ldx + c;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const bool ok = kvalid && ((rmask[i] >> tap_i) & 1u);
      hdu_bufload_lds16(xsrd, ok ? (unsigned)(rpix[i] + toff) * (unsigned)sizeof(T) : HDU_OOB, As + (i * RP + wave * 8) * 128);
    }
#pragma unroll
    for (int j = 0; j < B_IT; ++j) {
      if (j * RP + wave * 8 < BN)       // wave-uniform
        hdu_bufload_lds16(wsrd, (wrow[j] >= 0 && k < p.Ktot) ? (unsigned)(wrow[j] + k) * (unsigned)sizeof(T) : HDU_OOB,
                          Bs + (j * RP + wave * 8) * 128);
    }
    // advance to the next stage's position
    if (++l_kt == nk) {
      l_kt = 0;
      k_reset();
      const int prev_mt = l_mt;
      item_pos(++l_it, l_mt, l_nt);
      if (l_mt != prev_mt) tile_state();
      n_state();
    } else {
      k += BK;
      c += BK;
      while (c >= p.Cin) {
        c -= p.Cin;
        ++tap_i;
        if (++kw == p.KW) {
          kw = 0;
          if (++kh == p.KH) {
            kh = 0;
            ++kd;
          }
        }
      }
    }
  };
  tile_state();
  n_state();
  k_reset();
  issue(0);
  issue(1);

  // ---- COMPUTE side
  const unsigned dseed = p.drop_seed + (p.drop_seed_dev ? *p.drop_seed_dev : 0u);
  const bool has_bias = p.bias != nullptr, drop = p.drop_scale != 0.f, has_epi = p.epi_a != nullptr;
  T* __restrict__ yp = (T*)p.y;
  int slot = 0;
  for (int it = 0; it < nitems; ++it) {
    int mt, nt;
    item_pos(it, mt, nt);
    {
      f32x4 acc[TM][TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kt = 0; kt < nk; ++kt) {
        // stage `slot` has landed once at most ONE younger stage's DMAs of this wave are outstanding (epilogue stores share
        // the counter and only make the wait more conservative: loads return in order among themselves)
        if (nb_w == B_IT) hdu_wait_vmcnt_n<A_IT + B_IT>(); else hdu_wait_vmcnt_n<A_IT + B_IT - 1>();
        HDU_RAW_BARRIER();                       // everyone's part has landed; everyone is done reading the slot refilled next
        // the two waves of a SIMD (w, w + 4) take the step's two phases in OPPOSITE order, so that one requests the next
        // stage while the other multiplies (in lock step both would queue on the memory pipe, then both on the MFMA pipe)
        const bool issue_first = wave < 4 || (p.debug_flags & 64);
        if (issue_first) issue(slot == 0 ? NS - 1 : slot - 1);    // slot (s + NS - 1) % NS
        const char* As = smem + slot * STAGE;
        const char* Bs = As + BM * 128;
#pragma unroll
        for (int kg = 0; kg < 2; ++kg) {
          u32x4 af[TM], bf[TN];
          const int chunk = kg * 4 + (lane >> 4);
#pragma unroll
          for (int i = 0; i < TM; ++i) af[i] = *(const u32x4*)(As + lds_chunk_off(wave * WM + i * 16 + (lane & 15), chunk));
#pragma unroll
          for (int j = 0; j < TN; ++j) bf[j] = *(const u32x4*)(Bs + lds_chunk_off(j * 16 + (lane & 15), chunk));
          if constexpr (PRO) {
            const int cb = kt * BK + chunk * CH;
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = pro_apply<T>(af[i], pro_ta + cb, pro_tb + cb, pro_lo);
          }
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = Mma<T>::kgroup(bf[j], af[i], acc[i][j]);   // swapped: lane = 4 channels of one pixel
        }
        if (!issue_first) issue(slot == 0 ? NS - 1 : slot - 1);
        slot = slot == NS - 1 ? 0 : slot + 1;
      }
      // ---- epilogue in registers: C[m = lane & 15][n = 4 * (lane >> 4) + r] of each 16 x 16 fragment
      const int n0 = nt * BN;
      float* sdst = p.stats_partial ? p.stats_partial + (long long)((unsigned)mt % (unsigned)p.stats_slots) * 2 * p.Cout : nullptr;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + j * 16 + (lane >> 4) * 4;
        const bool n_ok = n < p.Cout;                 // Cout is a multiple of the 16-byte chunk: 4 channels are all-or-nothing
        const int nc = n_ok ? n : 0;
        const f32x4 bias_v = has_bias ? *(const f32x4*)(p.bias + nc) : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 epa_v = has_epi ? *(const f32x4*)(p.epi_a + nc) : f32x4{1.f, 1.f, 1.f, 1.f};
        const f32x4 epb_v = has_epi ? *(const f32x4*)(p.epi_b + nc) : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 sh_v = sdst ? *(const f32x4*)(p.stats_shift + nc) : f32x4{0.f, 0.f, 0.f, 0.f};
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const long long m = (long long)mt * BM + wave * WM + i * 16 + (lane & 15);
          const bool ok = n_ok && m < p.M;
          T* dst = yp + (ok ? m * p.ldy + n : 0);
          float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
          if (has_bias) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += bias_v[r];
          }
          if (drop) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const unsigned h = hdu_hash32((unsigned long long)m * (unsigned)p.Cout + (unsigned)(n + r), dseed);
              v[r] = h < p.drop_thresh ? v[r] * p.drop_scale : 0.f;
            }
          }
          if (has_epi) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              v[r] = epa_v[r] * v[r] + epb_v[r];
              if (p.epi_relu) v[r] = v[r] > 0.f ? v[r] : 0.f;
            }
          }
          if (p.accumulate) {                       // unconditional load at a clamped address (see bnb_issue_loads)
            float old[4];
            Chunk<T>::load4(dst, old);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += old[r];
          }
          if (ok) Chunk<T>::store4(dst, v);
          if (sdst) {                               // moments of the STORED values (what the consumers read)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float d = ok ? Chunk<T>::rounded(v[r]) - sh_v[r] : 0.f;
              s1[r] += d;
              s2[r] += d * d;
            }
          }
        }
        if (sdst) {
#pragma unroll
          for (int r = 0; r < 4; ++r) { s1[r] = hdu_row16_sum(s1[r]); s2[r] = hdu_row16_sum(s2[r]); }
          // every lane of a 16-lane group holds the group's 8 totals: lane q of the group adds total q
          const int q = lane & 15;
          float mine = 0.f;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            mine = q == r ? s1[r] : mine;
            mine = q == 4 + r ? s2[r] : mine;
          }
          if (q < 8 && n_ok) atomicAdd(sdst + (q < 4 ? 0 : p.Cout) + n + (q & 3), mine);
        }
      }
    }
  }
  HDU_WAIT_VMCNT(0);          // the two stages still in flight write LDS: they must land before the workgroup retires
}

// =====================================================================================
// Pointwise GEMM with a SHORT contraction and a WIDE output -- filter-stationary streaming form.
// The data gradient of every dense-block bottleneck (denseunet.py:245-248 / denseunet3d.py:34-37 backward):
//   dx[M x c] = dt[M x 192] . W^T,  c = 96 .. 2160 channels, K = 192 (2D) / 128 (3D) = 3 / 2 steps of 64.
// In the tiled kernels above every 64 x 128 output tile is its own workgroup: row state, a 2-3 step K loop and an
// epilogue -- ~11 us of fixed cost for ~1 us of multiplication (measured: 46 us per launch at M = 8192, 0.4 TB/s, 3.4 ms
// of the 21 ms 2D step).  Here a workgroup OWNS 128 output channels: their filter rows (128 x K, 48 KB) go to LDS once,
// then it streams its share of the pixel rows through a 3-slot ring of [64 rows x K] tiles (async buffer DMA, counted
// vmcnt, one raw barrier per tile) and writes each 64 x 128 result through a per-wave LDS staging patch as full 128-byte
// lines.  Waves: 2 (pixels) x 2 (channels), 32 x 64 outputs each -- a wave's staging rows are whole cache lines, so the
// epilogue needs no workgroup barrier.  Traffic per output element: the activation tile once per 128 channels, the filter
// once per workgroup.
// BNB (round 4): the launch is the data gradient of a bottleneck whose INPUT went through BN(+Scale)+ReLU (ConvK::bnb_*): the
// staged dz patch is turned into a * g (g = dz masked by the forward ReLU, recomputed from the BN input u) and stored / added
// straight onto the gradient slab, and S1 = sum g, S2 = sum g * uhat accumulate in registers over ALL tiles of the workgroup (a
// lane owns the same 8 channels for the whole launch) -- one set of float atomics per wave at the end.  The u / old-gradient
// chunks of a tile are requested before its MFMAs (and before the next operand tile's DMAs, so that the counted waits hold).
// This is the streaming form of epilogue_bn_backward: the dz round trip and the separate reduction + apply passes over the
// O(L^2)-wide slab go (14 -> 6 bytes per element); the reduction-dependent part of du follows later as -k3 * u + k4
// (hdu_bn_bwd_finalize / hdu_bn_bwd_correct).
template <int KS, int BN, bool BNB = false, int NSA = 3>
__global__ __launch_bounds__(256) void conv_pw_bstat_kernel(ConvK p, int rows_per_wg) {
  typedef bf16_t T;
  constexpr int CH = 8, BM = 64;
  constexpr int PD = NSA - 1;                          // every memory stream of the tile loop runs PD tiles ahead
  constexpr int A_SLAB = BM * 128, A_STAGE = KS * A_SLAB;
  constexpr int B_SLAB = BN * 128, B_BYTES = KS * B_SLAB;
  constexpr int WM = 32, WN = BN / 2, TM = WM / 16, TN = WN / 16;
  // (the 64-channel two-stage form fits two workgroups per CU in exactly 80 KB of LDS each: no bank padding of its patch rows)
  constexpr int CROWB = WN * 2 + (BN == 64 && NSA == 2 ? 0 : 16), CST = WM * CROWB;
  static_assert(NSA == 2 || NSA == 3, "ring depth");
  constexpr int A_IT = BM / 32, B_IT = BN / 32, LA = KS * A_IT;
  static_assert(BN % 64 == 0 && KS >= 1 && KS <= 4, "shape");
  static_assert(B_BYTES + NSA * A_STAGE + 4 * CST <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[B_BYTES + NSA * A_STAGE + 4 * CST];
  char* Bsm = smem;
  char* Aring = smem + B_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
#ifdef HDU_EMU
  const int wave = tid >> 6;
#else
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#endif
  const int wm = wave >> 1, wn = wave & 1;
  char* stg = smem + B_BYTES + NSA * A_STAGE + wave * CST;
  const int r0 = tid >> 3;
  const int kcl = (tid & 7) ^ (r0 & 7);          // logical 16-byte chunk of the 128-byte slab row this lane fetches
  // workgroup -> (row range, channel group), XCD-major (round 6): the gridDim.y channel-group workgroups of ONE row range read the same
  // dt tiles, and with the row-range index fastest in the dispatch order they landed on up to 8 different XCDs -- each XCD's L2 fetched
  // its own copy of every tile.  xcd_tile_index gives each XCD a contiguous range of (row range, channel group) pairs, channel groups
  // fastest (HDU_TUNE_DEBUG bit 11 restores the dispatch order)
  unsigned brow = blockIdx.x, bcol = blockIdx.y;
  if (!(p.debug_flags & 2048)) {
    const unsigned lin = blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned tix = xcd_tile_index(lin, gridDim.x * gridDim.y);
    bcol = tix % gridDim.y;
    brow = tix / gridDim.y;
  }
  const int n0 = (int)bcol * BN;
  const long long m_begin = (long long)brow * rows_per_wg;
  long long m_end = m_begin + rows_per_wg;
  if (m_end > p.M) m_end = p.M;
  const int ntiles = (int)((m_end - m_begin + BM - 1) / BM);
  if (ntiles <= 0) return;
  const hdu_bufsrd xsrd = hdu_make_srd(p.x, p.x_bytes);
  const hdu_bufsrd wsrd = hdu_make_srd(p.w, p.w_bytes);

  // ---- the filter rows of this workgroup's channels: once
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int j = 0; j < B_IT; ++j) {
      const int col = n0 + r0 + j * 32;
      const unsigned off = col < p.Cout ? (unsigned)(col * p.Ktot + ks * 64 + kcl * CH) * 2u : HDU_OOB;
      hdu_bufload_lds16(wsrd, off, Bsm + ks * B_SLAB + (j * 32 + wave * 8) * 128);
    }
  auto issue_tile = [&](int t) {
    char* As = Aring + (t % NSA) * A_STAGE;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const long long m = m_begin + (long long)t * BM + r0 + i * 32;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const unsigned off = m < m_end ? (unsigned)((unsigned long long)m * (unsigned long long)p.ldx + ks * 64 + kcl * CH) * 2u : HDU_OOB;
        hdu_bufload_lds16(xsrd, off, As + ks * A_SLAB + (i * 32 + wave * 8) * 128);
      }
    }
  };
  T* __restrict__ yp = (T*)p.y;
  // ---- BNB: this lane's 8 output channels are the same for every tile: coefficients once, S1 / S2 in registers
  constexpr int NCCE = WN / CH;                        // 16-byte chunks per row of a wave's patch (8)
  constexpr int EIT = WM * NCCE / 64;                  // chunks per lane and tile (4; 2 in the 64-channel form)
  static_assert(EIT == 4 || EIT == 2, "the counted waits below name four / two registers per operand");
  const int ecc = lane % NCCE;
  const int en = n0 + wn * WN + ecc * CH;
  const bool en_ok = en < p.Cout;
  float ba[CH], bb[CH], bmu[CH], brs[CH], bs1[CH], bs2[CH];
  const bool bsums = BNB && p.bnb_partial != nullptr;
  if constexpr (BNB) {
    const int nc = en_ok ? en : 0;
    const float* pmu = bsums ? p.bnb_mean : p.bnb_a;
    const float* prs = bsums ? p.bnb_rstd : p.bnb_a;
#pragma unroll
    for (int j = 0; j < CH; j += 4) {
      const f32x4 va = *(const f32x4*)(p.bnb_a + nc + j), vb = *(const f32x4*)(p.bnb_b + nc + j);
      const f32x4 vm = *(const f32x4*)(pmu + nc + j), vr = *(const f32x4*)(prs + nc + j);
#pragma unroll
      for (int r = 0; r < 4; ++r) { ba[j + r] = va[r]; bb[j + r] = vb[r]; bmu[j + r] = bsums ? vm[r] : 0.f; brs[j + r] = bsums ? vr[r] : 0.f; }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) { bs1[j] = 0.f; bs2[j] = 0.f; }
  }
  const T* __restrict__ bup = (const T*)p.bnb_u;

  // Round 6 -- the tile loop is SOFTWARE-PIPELINED over its memory round trips.  Round 5's loop requested a tile's u / old-gradient
  // chunks at the top of the tile with plain loads and stored at its end; hipcc's waitcnt bookkeeping then closed every tile with
  // s_waitcnt vmcnt(0) (ISA, tools/disasm_kernel.py).  Measured (tools/bench_pw_bstat.py, M = 8192, C = 1584): the plain form
  // (operand ring only, prefetch distance 2) takes 1.9 us per 64-row tile, the BN-backward form 3.3 us -- one loaded memory round
  // trip (~3 us) per tile: the kernel is bound by the bytes it keeps in flight per CU (Little's law), not by HBM (0.33 of its roof).
  // Now every memory stream of the loop runs TWO tiles ahead.  Per tile t (after its barrier):
  //   1. the stores of tile t-1 are issued (their values waited in registers: the acknowledgements have a whole tile to come back),
  //   2. the u / old chunks of tile t+2 are requested with loads the compiler does not count (HDU_ASYNC_LOAD16) into the register set
  //      tile t-1 used (three sets, the loop is unrolled by three: no copies of registers whose loads are in flight),
  //   3. the operand DMAs of tile t+2 are issued (dead -- zero-filling a free ring slot -- past the last tile: the counts are uniform),
  //   4. tile t is multiplied, staged, and its epilogue waits for ITS chunks with a counted vmcnt.
  // Counted waits (loads -- register or LDS-DMA -- retire in order among themselves, so a bound that counts only the LOADS issued
  // after the wanted ones holds whatever the stores in between do): top of tile t: the DMAs of tile t are followed by
  // [chunks t+1, DMAs t+1] = 2 EIT + LA loads; epilogue of tile t: its chunks are followed by [DMAs t] [chunks t+1, DMAs t+1]
  // [chunks t+2, DMAs t+2] = 3 LA + 4 EIT loads.
  // (u and y are addressed through raw buffer resources with 32-bit byte offsets -- launch precondition: both tensors end below
  // 4 GiB of their base, pw_bstat_ok -- so that a chunk in flight costs its data registers only: three sets must not spill)
  u32x4 uS[NSA][EIT], oS[NSA][EIT];                    // u / old-gradient chunks of the tiles t % NSA == 0 / 1 (/ 2)
  u32x4 pst[EIT];                                      // the finished output chunks of the previous tile
  unsigned poff[EIT];                                  // ... and where they go (HDU_OOB: nowhere)
#pragma unroll
  for (int it = 0; it < EIT; ++it) { poff[it] = HDU_OOB; pst[it] = u32x4{0u, 0u, 0u, 0u}; }
  const hdu_rawsrd ysrd = hdu_make_rawsrd(p.y, (unsigned)(((p.M - 1) * p.ldy + p.Cout) * 2));
  const hdu_rawsrd usrd = hdu_make_rawsrd(BNB ? p.bnb_u : p.y, (unsigned)(((p.M - 1) * (BNB ? p.bnb_ldu : p.ldy) + p.Cout) * 2));
  const unsigned ldu2 = (unsigned)p.bnb_ldu * 2u, ldy2 = (unsigned)p.ldy * 2u;
  const int erow = lane / NCCE;                         // this lane's row of the wave's patch in chunk round 0 (rounds are 64 / NCCE rows apart)
  auto issue_chunks = [&](int t, u32x4 (&uv)[EIT], u32x4 (&ov)[EIT]) {      // unconditional: a lane without a chunk reads zeros
#pragma unroll
    for (int it = 0; it < EIT; ++it) {
      const long long m = m_begin + (long long)t * BM + wm * WM + erow + it * (64 / NCCE);
      const bool ok = en_ok && m < m_end;
      const unsigned uoff = ok ? (unsigned)m * ldu2 + (unsigned)en * 2u : HDU_OOB;
      const unsigned ooff = (ok && p.accumulate) ? (unsigned)m * ldy2 + (unsigned)en * 2u : HDU_OOB;
      HDU_ASYNC_BUFLOAD16(uv[it], usrd, uoff);
      HDU_ASYNC_BUFLOAD16(ov[it], ysrd, ooff);
    }
  };
  // prologue, in the loop's issue order: [chunks 0, DMA tile 0] ([chunks 1, DMA tile 1])
  if constexpr (BNB) issue_chunks(0, uS[0], oS[0]);
  issue_tile(0);
  if constexpr (PD == 2) {
    if constexpr (BNB) issue_chunks(1, uS[1], oS[1]);
    issue_tile(1);
  }

  auto tile = [&](int t, u32x4 (&cuv)[EIT], u32x4 (&cov)[EIT], u32x4 (&nuv)[EIT], u32x4 (&nov)[EIT]) {
    // the DMAs of tile t are followed by PD - 1 rounds of [chunks, DMAs]
    if constexpr (BNB) hdu_wait_vmcnt_n<(PD - 1) * (LA + 2 * EIT)>(); else hdu_wait_vmcnt_n<(PD - 1) * LA>();
    HDU_RAW_BARRIER();
#pragma unroll
    for (int it = 0; it < EIT; ++it) hdu_bufstore16(ysrd, poff[it], pst[it]);
    if constexpr (BNB) issue_chunks(t + PD, nuv, nov);     // into the set tile t-1 has just released
    issue_tile(t + PD);                                // refills the slot tile t-1 was read from (all reads are behind the barrier)
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* At = Aring + (t % NSA) * A_STAGE;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const char* As = At + ks * A_SLAB;
      const char* Bs = Bsm + ks * B_SLAB;
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        u32x4 af[TM], bf[TN];
        const int chunk = kg * 4 + (lane >> 4);
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = *(const u32x4*)(As + lds_chunk_off(wm * WM + i * 16 + (lane & 15), chunk));
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = *(const u32x4*)(Bs + lds_chunk_off(wn * WN + j * 16 + (lane & 15), chunk));
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = Mma<T>::kgroup(bf[j], af[i], acc[i][j]);   // swapped: a lane holds 4 channels of one pixel
      }
    }
    // ---- epilogue of the tile: this wave's 32 x WN patch through its own LDS rows, out as 16-byte chunks of full lines
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
        Chunk<T>::store4((T*)(stg + (i * 16 + (lane & 15)) * CROWB) + j * 16 + (lane >> 4) * 4, v);
      }
    HDU_WAVE_LDS_SYNC();
    if constexpr (BNB) {
      // this tile's chunks are followed by [DMAs t] and PD rounds of [chunks, DMAs]
      constexpr int NUSE = LA + PD * (LA + 2 * EIT);
      if constexpr (EIT == 4) {
        hdu_wait_vmcnt_regs4<NUSE>(cuv[0], cuv[1], cuv[2], cuv[3]);
        hdu_wait_vmcnt_regs4<NUSE>(cov[0], cov[1], cov[2], cov[3]);
      } else {
        hdu_wait_vmcnt_regs4<NUSE>(cuv[0], cuv[1], cov[0], cov[1]);
      }
    }
#pragma unroll
    for (int it = 0; it < EIT; ++it) {
      const int q = lane + it * 64;
      const int row = q / NCCE, cc = q % NCCE;
      const long long m = m_begin + (long long)t * BM + wm * WM + row;
      const int n = n0 + wn * WN + cc * CH;
      const u32x4 v = *(const u32x4*)(stg + row * CROWB + cc * 16);
      const bool ok = m < m_end && n < p.Cout;
      poff[it] = ok ? (unsigned)m * ldy2 + (unsigned)n * 2u : HDU_OOB;
      if constexpr (BNB) {
        float dz[CH], u[CH], o[CH];
        Chunk<T>::unpack(v, dz);
        Chunk<T>::unpack(cuv[it], u);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const float sj = ba[j] * u[j] + bb[j];
          const float g = (ok && (!p.bnb_relu || sj > 0.f)) ? dz[j] : 0.f;
          bs1[j] += g;
          bs2[j] += g * ((u[j] - bmu[j]) * brs[j]);
          o[j] = ba[j] * g;
        }
        if (p.accumulate) {
          float old[CH];
          Chunk<T>::unpack(cov[it], old);
#pragma unroll
          for (int j = 0; j < CH; ++j) o[j] += old[j];
        }
        pst[it] = Chunk<T>::pack(o);
      } else {
        pst[it] = v;
      }
    }
    HDU_WAVE_LDS_SYNC();                               // (the patch is rewritten only after the next tile's barrier + MFMAs)
  };
  if constexpr (NSA == 3) {
    for (int t = 0; t < ntiles; t += 3) {
      tile(t, uS[0], oS[0], uS[2], oS[2]);
      if (t + 1 < ntiles) tile(t + 1, uS[1], oS[1], uS[0], oS[0]);
      if (t + 2 < ntiles) tile(t + 2, uS[2], oS[2], uS[1], oS[1]);
    }
  } else {
    for (int t = 0; t < ntiles; t += 2) {
      tile(t, uS[0], oS[0], uS[1], oS[1]);
      if (t + 1 < ntiles) tile(t + 1, uS[1], oS[1], uS[0], oS[0]);
    }
  }
#pragma unroll
  for (int it = 0; it < EIT; ++it) hdu_bufstore16(ysrd, poff[it], pst[it]);
  hdu_wait_vmcnt_n<0>();                               // dead DMAs of the last tiles write LDS: they must land before the workgroup retires
  if constexpr (BNB) {
    if (bsums) {
      // lanes ecc, ecc + 8, ... of a wave own the same 8 channels: butterfly over lane bits 3..5, then lanes 0..7 add the wave's
      // 8 x 2 x 8 totals to this workgroup's slot row (the two pixel waves of a channel half meet in the atomics)
#pragma unroll
      for (int mask = NCCE; mask < 64; mask <<= 1) {
#pragma unroll
        for (int j = 0; j < CH; ++j) { bs1[j] += __shfl_xor(bs1[j], mask); bs2[j] += __shfl_xor(bs2[j], mask); }
      }
      float* dst = p.bnb_partial + (long long)(brow % (unsigned)p.bnb_slots) * 2 * p.Cout;
      if (lane < NCCE && en_ok) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          atomicAdd(dst + en + j, bs1[j]);
          atomicAdd(dst + p.Cout + en + j, bs2[j]);
        }
      }
    }
  }
}

// bf16 filter gradient, DMA + transpose-read form (operands need no arithmetic: materialised inputs).
// PW = point-wise (1x1x1, stride 1, no padding, no up-sampling): input pixel == output pixel, so the per-row
// (n, d, h, w) decode, the tap bounds tests and the per-step carry loops disappear from the K loop.
// NCT = filter-row tiles of BCO channels one workgroup accumulates over the SAME staged x tile (round 3): the activations are
// the large operand of a pointwise layer (M x Cin, Cin up to 2112, against M x 192 of dy), and with one BCO = 64 tile per
// workgroup every x tile was fetched by 3 workgroups; NCT = 3 reads it once (LDS per stage 16 + 3 x 8 KB, two workgroups
// per CU instead of three).
template <int BCO, bool PW, int NCT = 1>
__device__ __forceinline__ void wgrad_dma_body(const ConvK& p, float* __restrict__ dw, long long rows_per_split,
                                               unsigned bid, char* smem) {
  typedef bf16_t T;
  constexpr int CH = 8;
  constexpr int PX = 64;
  constexpr int BKC = 128;
  constexpr int XROWB = 256;
  constexpr int DROWB = 128;
  constexpr int TM = BCO / 16;
  constexpr int TN = 2;
  constexpr int STAGE = PX * (XROWB + NCT * DROWB);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
#ifdef HDU_EMU
  const int wave = tid >> 6;
#else
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#endif
  const T* __restrict__ xp = (const T*)p.x;
  const T* __restrict__ dyp = (const T*)p.y;
  const char* zero = (const char*)hdu_zero_page;
  const bool ups = (p.ud | p.uh | p.uw) != 0;

  unsigned wbx, wby, wbz;
  // (XCD-major order: the k-column workgroups of one pixel split share its dy tile in one XCD's L2 -- see wgrad_halo_body;
  // HDU_TUNE_DEBUG bit 8 restores the round-robin order)
  if (!(p.debug_flags & 256)) bid = xcd_tile_index(bid, (unsigned)(p.wg_gx * p.wg_gy * p.wg_gz));
  if (!wgrad_block(p, bid, &wbx, &wby, &wbz)) return;
  const int kcol0 = (int)wbx * BKC;
  const int co0 = (int)wby * BCO * NCT;
  const long long m_begin = (long long)wbz * rows_per_split;
  long long m_end = m_begin + rows_per_split;
  if (m_end > p.M) m_end = p.M;

  // x tile: lane owns physical 16-byte chunk (tid&15) of pixel rows (tid>>4)+16*i; logical chunk via the swizzle
  const int pxl = tid >> 4;
  const int fx = (pxl & 3) | ((pxl >> 1) & 4);
  const int xp16 = tid & 15;
  const int kcc = ((((xp16 >> 1) ^ fx) << 1) | (xp16 & 1));
  const int kk = kcol0 + kcc * CH;
  const bool kvalid = kk < p.Ktot;
  int c = 0, kd = 0, kh = 0, kw = 0;
  if (kvalid) {
    const int tap = kk / p.Cin;
    c = kk - tap * p.Cin;
    kw = tap % p.KW;
    const int t = tap / p.KW;
    kh = t % p.KH;
    kd = t / p.KH;
  }
  int sn[4], sod[4], soh[4], sow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (PW) { sn[i] = sod[i] = soh[i] = sow[i] = 0; continue; }
    const long long m = m_begin + pxl + i * 16;
    const unsigned mu = (unsigned)m;                      // M < 2^31 (checked on the host): 32-bit divisions
    const int ow = (int)(mu % (unsigned)p.Wo);
    unsigned t = mu / (unsigned)p.Wo;
    const int oh = (int)(t % (unsigned)p.Ho);
    t /= (unsigned)p.Ho;
    sod[i] = (int)(t % (unsigned)p.Do);
    sn[i] = (int)(t / (unsigned)p.Do);
    soh[i] = oh;
    sow[i] = ow;
  }
  // dy tile: lane owns physical chunk (tid&7) of pixel rows (tid>>3)+32*j
  const int dpx0 = tid >> 3;
  const int gd = ((dpx0 >> 1) & 1) | (((dpx0 >> 3) & 1) << 1);
  const int dp16 = tid & 7;
  const int dcl = ((((dp16 >> 1) ^ gd) << 1) | (dp16 & 1));
  bool dvalid[NCT];
#pragma unroll
  for (int t = 0; t < NCT; ++t) dvalid[t] = dcl * CH < BCO && co0 + t * BCO + dcl * CH < p.Cout;

  auto issue_tile = [&](int buf, long long mt) {
    char* Xt = smem + buf * STAGE;
    char* Dt = Xt + PX * XROWB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long m = mt + pxl + i * 16;
      const char* g;
      if (PW) {
        g = (kvalid && m < m_end) ? (const char*)(xp + m * p.ldx + c) : zero;
      } else {
        const int id = sod[i] * p.sd - p.pd + kd, ih = soh[i] * p.sh - p.ph + kh, iw = sow[i] * p.sw - p.pw + kw;
        const bool ok = kvalid && m < m_end && (unsigned)id < (unsigned)p.De && (unsigned)ih < (unsigned)p.He &&
                        (unsigned)iw < (unsigned)p.We;
        const int src = ups ? ((sn[i] * p.Di + (id >> p.ud)) * p.Hi + (ih >> p.uh)) * p.Wi + (iw >> p.uw)
                            : ((sn[i] * p.De + id) * p.He + ih) * p.We + iw;
        g = ok ? (const char*)(xp + (long long)src * p.ldx + c) : zero;
      }
      hdu_glds16(g, Xt + (i * 16 + wave * 4) * XROWB);
    }
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const long long m = mt + dpx0 + j * 32;
        const char* g = (dvalid[t] && m < m_end) ? (const char*)(dyp + m * p.ldy + co0 + t * BCO + dcl * CH) : zero;
        hdu_glds16(g, Dt + t * (PX * DROWB) + (j * 32 + wave * 8) * DROWB);
      }
  };

  auto advance_pixels = [&]() {
    if (PW) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sow[i] += PX;
      while (sow[i] >= p.Wo) {
        sow[i] -= p.Wo;
        if (++soh[i] == p.Ho) {
          soh[i] = 0;
          if (++sod[i] == p.Do) {
            sod[i] = 0;
            ++sn[i];
          }
        }
      }
    }
  };

  f32x4 acc[NCT][TM][TN];
#pragma unroll
  for (int t = 0; t < NCT; ++t)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nsteps = (int)((m_end - m_begin + PX - 1) / PX);
  if (nsteps > 0) issue_tile(0, m_begin);
  const int li = lane & 15, lg = lane >> 4;
  // Pointwise layer whose input is relu(a[c] * x + b[c]) of the stored tensor (ConvK::pro_*: the dense-block bottlenecks read
  // the raw slab, see pro_apply above): after the transposing LDS read a lane's B fragment is 8 consecutive PIXELS of ONE
  // channel -- wave * 32 + j * 16 + li of this k-column tile --, so the affine is two per-lane scalars per fragment, loaded
  // once.  Pixels past m_end arrive as zeros and leave as relu(b): they meet zero dy rows.
  const bool has_pro = PW && p.pro_a != nullptr;
  float pro_a[TN], pro_b[TN];
  const float pro_lo = p.pro_relu ? 0.f : -__builtin_huge_valf();
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int ch = kcol0 + wave * 32 + j * 16 + li;
    const bool ok = has_pro && ch < p.Cin;
    pro_a[j] = ok ? p.pro_a[ch] : 0.f;
    pro_b[j] = ok ? p.pro_b[ch] : 0.f;
  }
  __syncthreads();
  for (int st = 0; st < nsteps; ++st) {
    const int buf = st & 1;
    if (st + 1 < nsteps) {
      advance_pixels();
      if (!(p.debug_flags & 1)) issue_tile(buf ^ 1, m_begin + (long long)(st + 1) * PX);
    }
    if (!(p.debug_flags & 2)) {
      const char* Xt = smem + buf * STAGE;
      const char* Dt = Xt + PX * XROWB;
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        u32x4 af[TM], bf[TN];
        const int prow = kg * 32 + lg * 8 + (li >> 2);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int bc = (wave * 32 + j * 16 + (li & 3) * 4) * 2;
          const u32x2 lo = hdu_lds_tr16_b64(Xt + tr_off<XROWB>(prow, bc));
          const u32x2 hi = hdu_lds_tr16_b64(Xt + tr_off<XROWB>(prow + 4, bc));
          bf[j] = u32x4{lo.x, lo.y, hi.x, hi.y};
          if (has_pro) {                                   // wave-uniform
            float f[8];
            Chunk<T>::unpack(bf[j], f);
#pragma unroll
            for (int q = 0; q < 8; ++q) f[q] = fmaxf(pro_a[j] * f[q] + pro_b[j], pro_lo);
            bf[j] = Chunk<T>::pack(f);
          }
        }
#pragma unroll
        for (int t = 0; t < NCT; ++t) {
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const int bc = (i * 16 + (li & 3) * 4) * 2;
            const u32x2 lo = hdu_lds_tr16_b64(Dt + t * (PX * DROWB) + tr_off<DROWB>(prow, bc));
            const u32x2 hi = hdu_lds_tr16_b64(Dt + t * (PX * DROWB) + tr_off<DROWB>(prow + 4, bc));
            af[i] = u32x4{lo.x, lo.y, hi.x, hi.y};
          }
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[t][i][j] = Mma<T>::kgroup(af[i], bf[j], acc[t][i][j]);
        }
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int t = 0; t < NCT; ++t)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + t * BCO + i * 16 + (lane >> 4) * 4 + r;
        if (co >= p.Cout) continue;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int kcol = kcol0 + wave * 32 + j * 16 + (lane & 15);
          if (kcol < p.Ktot && !(p.debug_flags & 4)) atomicAdd(dw + (long long)co * p.Ktot + kcol, acc[t][i][j][r]);
        }
      }
}

// =====================================================================================
// Halo-tile filter gradient for 2D 3x3 -- and, as three plane-shifted 2D problems, 3D 3x3x3 -- stride-1 "same" convolutions (bf16).
// The im2col view used by conv_wgrad_dma_kernel re-loads every input pixel once per tap and the output gradient
// once per k-column tile: measured, that kernel is bound by L2->LDS DMA traffic.  Here a workgroup owns a spatial
// tile of 4 x 32 output pixels and 32 input channels: it DMAs the (4+2) x (32+2) input halo tile and the dy tile
// ONCE and forms all 9 taps from LDS (transpose reads at shifted pixel addresses), i.e. 9x the MFMA work per byte.
// Accumulators: 9 taps x [BCO x 32] per workgroup; wave w owns (tap, 16-channel tile) combos w, w+4, ... and all
// BCO/16 output-channel tiles, so each B fragment is reused BCO/16 times and each A fragment ~4.5 times.
template <int BCO>
__device__ __forceinline__ void wgrad_halo_body(const ConvK& p, float* __restrict__ dw, int tiles_per_split, unsigned bid,
                                                char* smem) {
  typedef bf16_t T;
  constexpr int TH = 4, TW = 32, HC = TW + 2, HP = (TH + 2) * HC;      // 204 halo pixels
  constexpr int HPP = 208;                                             // padded to 16-pixel DMA instructions
  constexpr int XBYTES = HPP * 64;                                     // 32 channels * 2 B per halo pixel
  constexpr int DROWB = 128;
  constexpr int DBYTES = TH * TW * DROWB;
  constexpr int STAGE = XBYTES + DBYTES;
  constexpr int TMc = BCO / 16;
  constexpr int NQ = 5;                                                // combos per wave (18 combos over 4 waves)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
#ifdef HDU_EMU
  const int wave = tid >> 6;
#else
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#endif
  unsigned wbx, wby, wbz;
  // the channel-chunk workgroups of ONE pixel split share its dy (and neighbouring x) lines: XCD-major order puts them on one
  // XCD's L2 (round 4, PMC: 10 % L2 hits and 6.8 GB of fabric traffic for ~1 GB of operands with the round-robin order;
  // profiles/r04_experiment_wgrad_xcd_order.txt).  HDU_TUNE_DEBUG bit 7 restores the round-robin order (A/B).
  if (!(p.debug_flags & 128)) bid = xcd_tile_index(bid, (unsigned)(p.wg_gx * p.wg_gy * p.wg_gz));
  if (!wgrad_block(p, bid, &wbx, &wby, &wbz)) return;
  const int c0 = (int)wbx * 32;
  const int co0 = (int)wby * BCO;
  const int H = p.He, W = p.We;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  // 3 x 3 x 3 layers (round 4): a depth tap kd pairs output plane d with input plane d + kd - 1, and for a fixed kd the nine
  // (kh, kw) taps are a 2D filter gradient between those planes.  The planes of the volume are the "images" here, the splits
  // of the spatial tiles come in KD groups (wbz = split * KD + kd: the three workgroups of a split are neighbours in the
  // launch order and share the dy tiles and two of their three x planes in L2), planes outside the volume load as zeros.
  // (depth "same": pd = 1, as many input as output planes; depth "valid": pd = 0 and two more input planes -- the depth-sharded
  // layers, whose halo planes are part of the stored input)
  const int KDn = p.KD, Dn = p.Do, Dx = p.De;
  const int kd = (int)(wbz % (unsigned)KDn);
  const int xshift = kd - p.pd;                           // input plane = output plane + xshift (2D: 0)
  const int tap0 = kd * 9;
  const int ntiles = p.N * Dn * tiles_y * tiles_x;
  const int t_begin = (int)(wbz / (unsigned)KDn) * tiles_per_split;
  int t_end = t_begin + tiles_per_split;
  if (t_end > ntiles) t_end = ntiles;

  // Round 4: this kernel was bound by ADDRESS ARITHMETIC, not by MFMAs or bytes (ISA of round 3: 440 VALU + 500 SALU per
  // 4 x 32-pixel tile and wave against 60 MFMAs -- three runtime divisions for the tile position, 64-bit addresses with a
  // zero-page select for each of the 8 DMAs, the swizzled LDS address of each of the 64 transposing reads recomputed per
  // tile).  Everything that depends on the lane only is now computed ONCE: operands arrive through buffer resources (a lane
  // adds its fixed element offset to the tile's base, out-of-range = zeros: hdu_platform.h), the tile position advances
  // incrementally, and the lane's 64 LDS read addresses are kept as 16-bit offsets, two per register.
  // Tensors of 4 GiB and more (round 5: the whole 512^3 volume on one GPU -- dy of 3dconv_up4 is 17 GB): `big` = the resources
  // are made PER TILE from the 64-bit address of the tile's input plane / output plane, and the lane offsets stay inside that
  // plane (host: a plane is < 2 GiB).  Tensors below 4 GiB keep ONE resource over the whole tensor (no per-tile SALU).
  const long long dy_bytes = (((long long)p.M - 1) * p.ldy + p.Cout) * 2;
  const bool big = p.x_bytes == 0u || p.x_bytes > 0xF0000000u || dy_bytes >= 0xF0000000ll;     // (256 MB of slack for the halo offsets of a tile)
  const hdu_bufsrd xsrd = hdu_make_srd(p.x, p.x_bytes);
  const hdu_bufsrd dsrd = hdu_make_srd(p.y, (unsigned)dy_bytes);
  const long long xplane_elems = (long long)p.Hi * p.Wi * p.ldx, dplane_elems = (long long)p.He * p.We * p.ldy;
  const unsigned xplane_bytes = (unsigned)((xplane_elems - p.ldx + p.Cin) * 2), dplane_bytes = (unsigned)((dplane_elems - p.ldy + p.Cout) * 2);
  // x halo tile: instruction jj = j * 4 + wave covers halo pixels jj * 16 .. + 15, 4 lanes (16-byte chunks) per pixel
  int xhr[4], xhc[4], xoff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int jj = j * 4 + wave;
    const int hp = jj * 16 + (lane >> 2);
    const int pc = lane & 3;                             // physical 16-byte chunk inside the pixel's 64 B
    const int lc = ((((pc >> 1) ^ ((hp >> 3) & 1)) << 1) | (pc & 1));
    const int hr = hp / HC, hc = hp - hr * HC;
    const bool st = jj < HPP / 16 && hp < HP && c0 + lc * 8 < p.Cin;
    xhr[j] = st ? hr : (1 << 20);                        // (a row far outside every image: never valid)
    xhc[j] = hc;
    // element offset from the tile's origin pixel in the STORED input.  A nearest-neighbour up-sampling in front of the conv
    // (p.uh / p.uw) is taken here: tile origins are multiples of 4 x 32, so floor((y0 + r) / 2) = y0 / 2 + floor(r / 2)
    xoff[j] = (((hr - 1) >> p.uh) * p.Wi + ((hc - 1) >> p.uw)) * (int)p.ldx + c0 + lc * 8;
  }
  // dy tile: lane owns physical chunk (tid & 7) of tile pixels (tid >> 3) + 32 j = (row j, column tid >> 3)
  const int dpx0 = tid >> 3;
  const int gd = ((dpx0 >> 1) & 1) | (((dpx0 >> 3) & 1) << 1);
  const int dp16 = tid & 7;
  const int dcl = ((((dp16 >> 1) ^ gd) << 1) | (dp16 & 1));
  const bool dvalid = dcl * 8 < BCO && co0 + dcl * 8 < p.Cout;
  const int doff0 = dpx0 * (int)p.ldy + co0 + dcl * 8;   // + j * W * ldy for tile row j

  // load-side tile position, advanced incrementally
  int l_tx, l_ty, l_n, l_d, l_v;
  {
    const int r = t_begin / tiles_x;
    l_tx = t_begin - r * tiles_x;
    l_n = r / tiles_y;
    l_ty = r - l_n * tiles_y;
    l_v = l_n / Dn;                                       // volume and depth plane of image l_n
    l_d = l_n - l_v * Dn;
  }
  auto issue_tile = [&](int buf) {
    char* Xh = smem + buf * STAGE;
    char* Dt = Xh + XBYTES;
    const int y0 = l_ty * TH, x0 = l_tx * TW;
    const bool plane_ok = (unsigned)(l_d + xshift) < (unsigned)Dx;
    const int xplane = l_v * p.Di + (plane_ok ? ((l_d + xshift) >> p.ud) : 0);          // stored input plane
    const int xin = ((y0 >> p.uh) * p.Wi + (x0 >> p.uw)) * (int)p.ldx;                 // tile origin inside the plane
    const int din = (y0 * W + x0) * (int)p.ldy;
    const hdu_bufsrd xs = big ? hdu_make_srd((const bf16_t*)p.x + (long long)xplane * xplane_elems, xplane_bytes) : xsrd;
    const hdu_bufsrd ds = big ? hdu_make_srd((const bf16_t*)p.y + (long long)l_n * dplane_elems, dplane_bytes) : dsrd;
    const int xbase = big ? xin : xplane * (int)xplane_elems + xin;                     // valid pixels give >= 0 sums
    const int dbase = big ? din : l_n * (int)dplane_elems + din;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int jj = j * 4 + wave;
      if (jj < HPP / 16) {                                  // wave-uniform
        const bool ok = plane_ok && (unsigned)(y0 - 1 + xhr[j]) < (unsigned)H && (unsigned)(x0 - 1 + xhc[j]) < (unsigned)W;
        hdu_bufload_lds16(xs, ok ? (unsigned)(xbase + xoff[j]) * 2u : HDU_OOB, Xh + jj * 1024);
      }
    }
    const bool colok = dvalid && x0 + dpx0 < W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = colok && y0 + j < H;
      hdu_bufload_lds16(ds, ok ? (unsigned)(dbase + j * W * (int)p.ldy + doff0) * 2u : HDU_OOB, Dt + (j * 32 + wave * 8) * DROWB);
    }
    if (++l_tx == tiles_x) {
      l_tx = 0;
      if (++l_ty == tiles_y) {
        l_ty = 0;
        ++l_n;
        if (++l_d == Dn) { l_d = 0; ++l_v; }
      }
    }
  };

  // ---- the lane's LDS read addresses (tile-invariant), relative to the stage base
  const int li = lane & 15, lg = lane >> 4, q4 = li >> 2;
  // dy fragment i, k-group kg, half h: pixel row kg * 32 + lg * 8 + q4 + 4 h; tr_off<128>'s swizzle bits depend on the lane only
  int dbase_i[TMc];
  {
    const int swz = ((q4 >> 1) & 1) | ((lg & 1) << 1);
#pragma unroll
    for (int i = 0; i < TMc; ++i) dbase_i[i] = XBYTES + (lg * 8 + q4) * DROWB + ((i ^ swz) << 5) + (li & 3) * 8;
  }
  // x fragment of combo (tap, ct), k-group kg, half h: halo pixel (kg + kh) * HC + kw + 4 h + lg * 8 + q4; its swizzle bit is
  // bit 3 of that ABSOLUTE pixel index, so the offsets are enumerated once: [q][kg][h] as 16-bit halves, two per register
  unsigned xadr[NQ][TH];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    // (waves 2 and 3 have no fifth combo: they multiply combo `wave` once more into an accumulator set nobody stores -- a
    // branch-free k loop lets every transposing read of a k-group be requested before its first MFMA; with the wave-uniform
    // `if (combo < 18)` of round 3 each pair of reads was followed by a full LDS round trip)
    const int combo = wave + 4 * q < 18 ? wave + 4 * q : wave;
    const int tap = combo >> 1, ct = combo & 1;
    const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
    for (int kg = 0; kg < TH; ++kg) {
      const int hp = (kg + kh) * HC + lg * 8 + q4 + kw;
      const int hp2 = hp + 4;
      const unsigned lo = (unsigned)(hp * 64 + ((ct ^ ((hp >> 3) & 1)) << 5) + (li & 3) * 8);
      const unsigned hi = (unsigned)(hp2 * 64 + ((ct ^ ((hp2 >> 3) & 1)) << 5) + (li & 3) * 8);
      xadr[q][kg] = lo | (hi << 16);                     // both < XBYTES = 13312
    }
  }

  f32x4 acc[NQ][TMc];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int i = 0; i < TMc; ++i) acc[q][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (t_begin < t_end) issue_tile(0);
  __syncthreads();
  for (int t = t_begin; t < t_end; ++t) {
    const int buf = (t - t_begin) & 1;
    if (t + 1 < t_end) issue_tile(buf ^ 1);
    {
      const char* St = smem + buf * STAGE;
#pragma unroll
      for (int kg = 0; kg < TH; ++kg) {                    // k-group = tile row kg: 32 pixels
        u32x4 af[TMc];
#pragma unroll
        for (int i = 0; i < TMc; ++i) {
          const char* a0 = St + dbase_i[i] + kg * 32 * DROWB;
          const u32x2 lo = hdu_lds_tr16_b64(a0);
          const u32x2 hi = hdu_lds_tr16_b64(a0 + 4 * DROWB);
          af[i] = u32x4{lo.x, lo.y, hi.x, hi.y};
        }
        u32x4 bf[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const unsigned pr = xadr[q][kg];
          const u32x2 lo = hdu_lds_tr16_b64(St + (pr & 0xffffu));
          const u32x2 hi = hdu_lds_tr16_b64(St + (pr >> 16));
          bf[q] = u32x4{lo.x, lo.y, hi.x, hi.y};
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
          for (int i = 0; i < TMc; ++i) acc[q][i] = Mma<T>::kgroup(af[i], bf[q], acc[q][i]);
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int combo = wave + 4 * q;
    if (combo >= 18) continue;
    const int tap = combo >> 1, ct = combo & 1;
    const int c = c0 + ct * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < TMc; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + i * 16 + (lane >> 4) * 4 + r;
        if (co < p.Cout && c < p.Cin) atomicAdd(dw + (long long)co * p.Ktot + (tap0 + tap) * p.Cin + c, acc[q][i][r]);
      }
  }
}

// ---- launch forms of the two bf16 filter-gradient bodies.  Single: one layer per launch (hdu_conv_wgrad).  Batched:
// one launch covers MANY layers (hdu_wgrad_plan_run): filter gradients feed nothing but the optimiser, so the engine
// defers them to the end of the backward pass; the late dense layers (2048..8192 pixels) that cannot fill the chip on
// their own then share it, and ~135 launches per step (ramp-up, tail, drain each) become a handful.
template <int BCO, bool PW, int NCT = 1>
__global__ __launch_bounds__(256) void conv_wgrad_dma_kernel(ConvK p, float* __restrict__ dw, long long rows_per_split) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 64 * (256 + NCT * 128)];
  wgrad_dma_body<BCO, PW, NCT>(p, dw, rows_per_split, blockIdx.x, smem);
}

template <int BCO>
__global__ __launch_bounds__(256) void conv_wgrad_halo_kernel(ConvK p, float* __restrict__ dw, int tiles_per_split) {
  __shared__ __attribute__((aligned(16))) char smem[2 * (208 * 64 + 4 * 32 * 128)];
  wgrad_halo_body<BCO>(p, dw, tiles_per_split, blockIdx.x, smem);
}

// workgroup -> (layer, workgroup within the layer): begins[i] = first workgroup of layer i, ascending
__device__ __forceinline__ int batched_find(const unsigned* __restrict__ begins, int n, unsigned bid) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (begins[mid] <= bid) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <int BCO, bool PW, int NCT = 1>
__global__ __launch_bounds__(256) void conv_wgrad_dma_batched_kernel(const WgradEntry* __restrict__ tab,
                                                                     const unsigned* __restrict__ begins, int n) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 64 * (256 + NCT * 128)];
  const int e = batched_find(begins, n, blockIdx.x);
  const ConvK p = tab[e].k;
  wgrad_dma_body<BCO, PW, NCT>(p, tab[e].dw, tab[e].per, blockIdx.x - begins[e], smem);
}

template <int BCO>
__global__ __launch_bounds__(256) void conv_wgrad_halo_batched_kernel(const WgradEntry* __restrict__ tab,
                                                                      const unsigned* __restrict__ begins, int n) {
  __shared__ __attribute__((aligned(16))) char smem[2 * (208 * 64 + 4 * 32 * 128)];
  const int e = batched_find(begins, n, blockIdx.x);
  const ConvK p = tab[e].k;
  wgrad_halo_body<BCO>(p, tab[e].dw, (int)tab[e].per, blockIdx.x - begins[e], smem);
}

// =====================================================================================
// Halo-tile forward / data-gradient GEMM for 2D 3x3 stride-1 "same" convolutions (bf16, DMA operands).
// Workgroup = 4 x 32 output pixels x BN output channels; K loop over 32-channel chunks.  Per chunk ONE DMA of the
// (4+2) x (32+2) input halo tile (64 B per pixel) and of the filters of all 9 taps for these 32 channels; the 9 taps
// are then formed from LDS (A fragments = shifted pixel windows of the halo tile).  L2->LDS traffic per MAC drops
// ~2.3x against the im2col tiling.  Wave w owns tile row w (two 16-pixel m-tiles) and all BN/16 n-tiles.
// LDS swizzle: the 16-byte chunk c of pixel/filter-row r is stored at chunk c ^ PI[(r >> 2) & 3], PI = {0,3,2,1}:
// the two row sets of a ds_read_b128 lane group ({0-3,12-15} with chunk g, {4-11} with chunk g+1) then cover all
// 16 bank slots.
__device__ __forceinline__ int halo_swz(int r) { return (0x6C >> (((r >> 2) & 3) * 2)) & 3; }   // {0,3,2,1}

template <int BN>
__global__ __launch_bounds__(256) void conv_halo_fprop_kernel(ConvK p) {
  typedef bf16_t T;
  constexpr int TH = 4, TW = 32, HC = TW + 2, HP = (TH + 2) * HC, HPP = 208;
  constexpr int XBYTES = HPP * 64;
  constexpr int WROWB = 9 * 64;                          // filter row: 9 taps x 32 channels x 2 B
  constexpr int WCH = BN * 36;                           // 16-byte chunks of the filter tile
  constexpr int W_IT = (WCH + 255) / 256;
  constexpr int WBYTES = ((WCH + 63) / 64) * 1024;       // whole wave instructions
  constexpr int STAGE = XBYTES + WBYTES;
  constexpr int TN = BN / 16;
  constexpr int BM = TH * TW;
  static_assert(2 * STAGE <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
#ifdef HDU_EMU
  const int wave = tid >> 6;
#else
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#endif
  const T* __restrict__ xp = (const T*)p.x;
  const T* __restrict__ wp = (const T*)p.w;
  const char* zero = (const char*)hdu_zero_page;
  const int H = p.He, W = p.We;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int t = blockIdx.x;
  const int txi = t % tiles_x;
  const int r_ = t / tiles_x;
  const int tyi = r_ % tiles_y;
  const int n = r_ / tiles_y;
  const int y0 = tyi * TH, x0 = txi * TW;
  const int n0 = blockIdx.y * BN;

  // ---- fixed DMA roles of this lane
  // halo tile: instruction jj = j*4 + wave covers halo pixels jj*16 .. +15
  const char* xsrc[4];
  int xlc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int jj = j * 4 + wave;
    const int hp = jj * 16 + (lane >> 2);
    const int lc = (lane & 3) ^ halo_swz(hp);
    const int hr = hp / HC, hc = hp - hr * HC;
    const int iy = y0 - 1 + hr, ix = x0 - 1 + hc;
    const bool ok = jj < HPP / 16 && hp < HP && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
    xsrc[j] = ok ? (const char*)(xp + ((long long)(n * H + iy) * W + ix) * p.ldx + lc * 8) : nullptr;
    xlc[j] = lc * 8;
  }
  // filter tile: flat chunk q = (row, tap, chunk-in-tap): instruction covers 64 consecutive chunks
  const char* wsrc[W_IT];
  int wlc[W_IT];
#pragma unroll
  for (int j = 0; j < W_IT; ++j) {
    const int q = (j * 4 + wave) * 64 + lane;
    const int row = q / 36, rem = q - row * 36;
    const int tap = rem >> 2;
    const int lc = (rem & 3) ^ halo_swz(row);
    const int co = n0 + row;
    const bool ok = q < WCH && co < p.Cout;
    wsrc[j] = ok ? (const char*)(wp + ((long long)co * 9 + tap) * p.Cin + lc * 8) : nullptr;
    wlc[j] = lc * 8;
  }

  auto issue_chunk = [&](int buf, int c0) {
    char* Xh = smem + buf * STAGE;
    char* Ws = Xh + XBYTES;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int jj = j * 4 + wave;
      if (jj < HPP / 16) {
        const char* g = (xsrc[j] != nullptr && c0 + xlc[j] < p.Cin) ? xsrc[j] + c0 * 2 : zero;
        hdu_glds16(g, Xh + jj * 1024);
      }
    }
#pragma unroll
    for (int j = 0; j < W_IT; ++j) {
      const int jj = j * 4 + wave;
      if (jj * 64 < WCH) {
        const char* g = (wsrc[j] != nullptr && c0 + wlc[j] < p.Cin) ? wsrc[j] + c0 * 2 : zero;
        hdu_glds16(g, Ws + jj * 1024);
      }
    }
  };

  f32x4 acc[2][TN];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunks = (p.Cin + 31) / 32;
  issue_chunk(0, 0);
  __syncthreads();
  const int li = lane & 15, lg = lane >> 4;
  for (int kc = 0; kc < nchunks; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nchunks) issue_chunk(buf ^ 1, (kc + 1) * 32);
    {
      const char* Xh = smem + buf * STAGE;
      const char* Ws = Xh + XBYTES;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int kh = tap / 3, kw = tap - kh * 3;
        u32x4 af[2], bf[TN];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int hp = (wave + kh) * HC + i * 16 + li + kw;
          af[i] = *(const u32x4*)(Xh + hp * 64 + ((lg ^ halo_swz(hp)) << 4));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int row = j * 16 + li;
          bf[j] = *(const u32x4*)(Ws + row * WROWB + tap * 64 + ((lg ^ halo_swz(row)) << 4));
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = Mma<T>::kgroup(bf[j], af[i], acc[i][j]);   // transposed tile: see igemm_epilogue
      }
    }
    __syncthreads();
  }

  // ---- epilogue: bias / dropout in registers, LDS-staged 16-byte row stores (tile pixel -> image pixel)
  constexpr int ROWB = BN * 2 + 16;
  const unsigned dseed = p.drop_seed + (p.drop_seed_dev ? *p.drop_seed_dev : 0u);
  const bool has_bias = p.bias != nullptr, drop = p.drop_scale != 0.f, has_epi = p.epi_a != nullptr;
  f32x4 bias_v[TN], epa_v[TN], epb_v[TN];            // loaded once, unconditionally (see igemm_epilogue)
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nn = n0 + j * 16 + lg * 4;
    const int nc = nn < p.Cout ? nn : 0;
    bias_v[j] = has_bias ? *(const f32x4*)(p.bias + nc) : f32x4{0.f, 0.f, 0.f, 0.f};
    epa_v[j] = has_epi ? *(const f32x4*)(p.epi_a + nc) : f32x4{1.f, 1.f, 1.f, 1.f};
    epb_v[j] = has_epi ? *(const f32x4*)(p.epi_b + nc) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {                      // (operands swapped in the K loop: lane = pixel li, 4 channels lg*4..)
    const int tx = i * 16 + li;
    const int row = wave * 32 + tx;
    const long long m = ((long long)(n * H + y0 + wave)) * W + x0 + tx;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = j * 16 + lg * 4;
      const int nn = n0 + col;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (has_bias) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += bias_v[j][r];
      }
      if (drop) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned h = hdu_hash32((unsigned long long)m * (unsigned)p.Cout + (unsigned)(nn + r), dseed);
          v[r] = h < p.drop_thresh ? v[r] * p.drop_scale : 0.f;
        }
      }
      if (has_epi) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = epa_v[j][r] * v[r] + epb_v[j][r];
          if (p.epi_relu) v[r] = v[r] > 0.f ? v[r] : 0.f;
        }
      }
      Chunk<T>::store4((T*)(smem + row * ROWB) + col, v);
    }
  }
  __syncthreads();
  T* __restrict__ yp = (T*)p.y;
  constexpr int NCC = BN / 8;
  for (int q = tid; q < BM * NCC; q += 256) {
    const int row = q / NCC, cc = q - row * NCC;
    const int oy = y0 + (row >> 5), ox = x0 + (row & 31);
    const int nn = n0 + cc * 8;
    if (oy >= H || ox >= W || nn >= p.Cout) continue;
    u32x4 v = *(const u32x4*)(smem + row * ROWB + cc * 16);
    T* dst = yp + (((long long)(n * H + oy)) * W + ox) * p.ldy + nn;
    if (p.accumulate) {
      float f[8], g[8];
      Chunk<T>::unpack(v, f);
      Chunk<T>::unpack(*(const u32x4*)dst, g);
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) f[jj] += g[jj];
      v = Chunk<T>::pack(f);
    }
    *(u32x4*)dst = v;
  }
  if (p.stats_partial)
    epilogue_stats<T, BM, BN, ROWB>(p, smem, n0, tid, blockIdx.x,
                                    [&](int row) { return y0 + (row >> 5) < H && x0 + (row & 31) < W; });
}

// =====================================================================================
// strided data gradient (only the stride-2 stems need it; tiny share of the FLOPs): direct gather form,
// one thread per (input pixel, 16-byte channel chunk).  w is the forward filter [Cout][T][Cin] in dtype T.
template <typename T>
__global__ __launch_bounds__(256) void conv_dgrad_strided_kernel(ConvK p) {
  constexpr int CH = Chunk<T>::CH;
  const int ncc = p.Cin / CH;
  const long long total = (long long)p.N * p.Di * p.Hi * p.Wi * ncc;
  const T* __restrict__ dyp = (const T*)p.y;
  const T* __restrict__ wp = (const T*)p.w;
  T* __restrict__ dxp = (T*)p.x;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    const int cc = (int)(q % ncc);
    long long pix = q / ncc;
    const int iw = (int)(pix % p.Wi);
    long long t = pix / p.Wi;
    const int ih = (int)(t % p.Hi);
    t /= p.Hi;
    const int id = (int)(t % p.Di);
    const int n = (int)(t / p.Di);
    float acc[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) acc[j] = 0.f;
    for (int kd = 0; kd < p.KD; ++kd) {
      const int td = id + p.pd - kd;
      if (td < 0 || td % p.sd) continue;
      const int od = td / p.sd;
      if (od >= p.Do) continue;
      for (int kh = 0; kh < p.KH; ++kh) {
        const int th = ih + p.ph - kh;
        if (th < 0 || th % p.sh) continue;
        const int oh = th / p.sh;
        if (oh >= p.Ho) continue;
        for (int kw = 0; kw < p.KW; ++kw) {
          const int tw = iw + p.pw - kw;
          if (tw < 0 || tw % p.sw) continue;
          const int ow = tw / p.sw;
          if (ow >= p.Wo) continue;
          const long long m = (((long long)n * p.Do + od) * p.Ho + oh) * p.Wo + ow;
          const int tap = (kd * p.KH + kh) * p.KW + kw;
          const T* dyr = dyp + m * p.ldy;
          const T* wr = wp + (long long)tap * p.Cin + cc * CH;
          for (int co = 0; co < p.Cout; ++co) {
            const float g = Chunk<T>::load1(dyr + co);
            float wv[CH];
            Chunk<T>::unpack(*(const u32x4*)(wr + (long long)co * p.Ktot), wv);
#pragma unroll
            for (int j = 0; j < CH; ++j) acc[j] += g * wv[j];
          }
        }
      }
    }
    T* o = dxp + pix * p.ldx + cc * CH;
    if (p.accumulate) {
      float old[CH];
      Chunk<T>::unpack(*(const u32x4*)o, old);
#pragma unroll
      for (int j = 0; j < CH; ++j) acc[j] += old[j];
    }
    *(u32x4*)o = Chunk<T>::pack(acc);
  }
}

// =====================================================================================
// filter preparation: float32 master [Cout][T][Cin] -> compute dtype forward copy (same layout) and the
// data-gradient filter [Cin][T flipped][Cout].
// ---- stride-2 data gradient as 2^d stride-1 implicit GEMMs (the 7x7x7 stride-2 stem of the end-to-end hybrid).
// dx[i] = sum_k dy[(i + p - k) / 2] * w[k] over the taps k with (i + p - k) even: input positions of parity r = i & 1 only
// see the taps k = kmax_r, kmax_r - 2, ... -- a stride-1 correlation of dy with a sub-filter of ceil/floor(K/2) taps per
// axis.  hdu_stride2_dgrad_filters gathers the 2^d sub-filters ([Cin][taps][Cout], the layout hdu_conv_fprop takes as a
// data-gradient filter), hdu_conv_fprop runs each class on the MFMA path, hdu_parity_interleave scatters the class
// outputs into dx.  Replaces the scalar gather kernel above on the hot path (9.7 ms -> ~1 ms per end2end step).
struct ParityGeom {
  int nt[3];        // taps per axis of this class
  int kmax[3];      // largest forward-filter tap of the class's parity: tap t of the sub-filter is k = kmax - step*t
  int step[3];      // 2 on a stride-2 axis, 1 on a stride-1 axis
  long long dst_off;
};
struct ParityTable { ParityGeom c[8]; int n; };

template <typename T>
__global__ __launch_bounds__(256) void stride2_filter_kernel(const float* __restrict__ wm, int Cout, int KD, int KH, int KW,
                                                            int Cin, ParityTable tab, T* __restrict__ out) {
  const ParityGeom g = tab.c[blockIdx.y];
  const long long total = (long long)Cin * g.nt[0] * g.nt[1] * g.nt[2] * Cout;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
    const int co = (int)(q % Cout);
    long long t = q / Cout;
    const int tw = (int)(t % g.nt[2]); t /= g.nt[2];
    const int th = (int)(t % g.nt[1]); t /= g.nt[1];
    const int td = (int)(t % g.nt[0]);
    const int ci = (int)(t / g.nt[0]);
    const int kd = g.kmax[0] - g.step[0] * td, kh = g.kmax[1] - g.step[1] * th, kw = g.kmax[2] - g.step[2] * tw;
    const float v = wm[((((long long)co * KD + kd) * KH + kh) * KW + kw) * Cin + ci];
    Chunk<T>::store1(out + g.dst_off + q, v);
  }
}

// dx[n][2qd+rd][2qh+rh][2qw+rw][c] (+)= cls[class(rd,rh,rw)][n][qd][qh][qw][c]; a stride-1 axis has one class (r = 0, q = i)
template <typename T>
__global__ __launch_bounds__(256) void parity_interleave_kernel(const T* __restrict__ cls, int N, int Di, int Hi, int Wi, int C,
                                                               int sd, int sh, int sw, T* __restrict__ dx, long long lddx,
                                                               int accumulate) {
  constexpr int CH = Chunk<T>::CH;
  const int ncc = C / CH;
  const long long total = (long long)N * Di * Hi * Wi * ncc;
  const int Dq = (Di + sd - 1) / sd, Hq = (Hi + sh - 1) / sh, Wq = (Wi + sw - 1) / sw;   // class grids (even dims: equal for all r)
  const long long cls_elems = (long long)N * Dq * Hq * Wq * C;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
    const int cc = (int)(q % ncc);
    long long pix = q / ncc;
    const int iw = (int)(pix % Wi);
    long long t = pix / Wi;
    const int ih = (int)(t % Hi);
    t /= Hi;
    const int id = (int)(t % Di);
    const int n = (int)(t / Di);
    const int rd = id % sd, rh = ih % sh, rw = iw % sw;
    const int ci = (rd * sh + rh) * sw + rw;
    const long long src = ci * cls_elems + ((((long long)n * Dq + id / sd) * Hq + ih / sh) * Wq + iw / sw) * C + cc * CH;
    u32x4 v = *(const u32x4*)(cls + src);
    T* o = dx + pix * lddx + cc * CH;
    if (accumulate) {
      float a[CH], b[CH];
      Chunk<T>::unpack(v, a);
      Chunk<T>::unpack(*(const u32x4*)o, b);
#pragma unroll
      for (int j = 0; j < CH; ++j) a[j] += b[j];
      v = Chunk<T>::pack(a);
    }
    *(u32x4*)o = v;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void weight_prep_kernel(const float* __restrict__ wm, int Cout, int Tn, int Cin,
                                                         T* __restrict__ wf, T* __restrict__ wd) {
  const long long total = (long long)Cout * Tn * Cin;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    const int ci = (int)(q % Cin);
    const long long t2 = q / Cin;
    const int t = (int)(t2 % Tn);
    const int co = (int)(t2 / Tn);
    const float v = wm[q];
    if (wf) Chunk<T>::store1(wf + q, v);
    if (wd) Chunk<T>::store1(wd + ((long long)ci * Tn + (Tn - 1 - t)) * Cout + co, v);
  }
}

// 64 x 64 (Cout x Cin) tiles of one tap of one layer: 16-byte reads of the float32 master along Cin, 8-byte (bf16) / 16-byte (float32)
// writes of the forward copy, LDS transpose, the same store width for the data-gradient copy along Cout.  tile_begin[] (in the
// table) maps a tile to its layer by binary search; a workgroup walks HDU_PREP_TPW consecutive tiles and searches once.
// Round 6: the 32 x 32 / one element per lane form of rounds 2-5 ran at 1.7-2.1 TB/s -- 2-byte stores, one per lane and element.
// Entries whose offsets or channel counts are not multiples of 4 take the element-wise path of the same tile (workgroup-uniform).
#define HDU_PREP_TPW 2
template <typename T>
__global__ __launch_bounds__(256) void weight_prep_batched_kernel(const hdu_prep_entry* __restrict__ table, int n,
                                                                 const float* __restrict__ master, T* __restrict__ wc,
                                                                 long long total_tiles) {
  __shared__ float tile[2][64][65];
  const long long t0 = (long long)blockIdx.x * HDU_PREP_TPW;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].tile_begin <= t0) lo = mid; else hi = mid - 1;
  }
  hdu_prep_entry e = table[lo];
  long long next_begin = lo + 1 < n ? table[lo + 1].tile_begin : total_tiles;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int it = 0; it < HDU_PREP_TPW; ++it) {
    const long long t = t0 + it;
    if (t >= total_tiles) break;
    while (t >= next_begin) {                // (workgroup-uniform)
      ++lo;
      e = table[lo];
      next_begin = lo + 1 < n ? table[lo + 1].tile_begin : total_tiles;
    }
    const int t_local = (int)(t - e.tile_begin);
    const int nci = (e.Cin + 63) / 64, nco = (e.Cout + 63) / 64;
    const int cib = t_local % nci;
    const int cob = (t_local / nci) % nco;
    const int tap = t_local / (nci * nco);
    const float* wm = master + e.master_off;
    T* wf = e.w_f_off >= 0 ? wc + e.w_f_off : nullptr;
    T* wd = e.w_d_off >= 0 ? wc + e.w_d_off : nullptr;
    float (*tl)[65] = tile[it & 1];          // two buffers: ONE barrier per tile (the next tile's fill cannot overtake this tile's reads)
    const bool vec = ((e.master_off | (e.w_f_off >= 0 ? e.w_f_off : 0) | (e.w_d_off >= 0 ? e.w_d_off : 0) | (long long)e.Cin | (long long)e.Cout) & 3) == 0 &&
                     (((uintptr_t)master | (uintptr_t)wc) & 15) == 0;
    if (vec) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int r = ty + 16 * k;
        const int co = cob * 64 + r, ci = cib * 64 + tx * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (co < e.Cout && ci < e.Cin) {       // (Cin a multiple of 4: the quad is inside the row)
          const long long q = ((long long)co * e.T + tap) * e.Cin + ci;
          const f32x4 m = *(const f32x4*)(wm + q);
          v[0] = m.x; v[1] = m.y; v[2] = m.z; v[3] = m.w;
          if (wf) Chunk<T>::store4(wf + q, v);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) tl[r][tx * 4 + j] = v[j];
      }
      __syncthreads();
      if (wd) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int r = ty + 16 * k;
          const int ci = cib * 64 + r, co = cob * 64 + tx * 4;
          if (co < e.Cout && ci < e.Cin) {
            const float v[4] = {tl[tx * 4 + 0][r], tl[tx * 4 + 1][r], tl[tx * 4 + 2][r], tl[tx * 4 + 3][r]};
            Chunk<T>::store4(wd + ((long long)ci * e.T + (e.T - 1 - tap)) * e.Cout + co, v);
          }
        }
      }
    } else {
      for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        const int co = cob * 64 + r, ci = cib * 64 + c;
        float v = 0.f;
        if (co < e.Cout && ci < e.Cin) {
          const long long q = ((long long)co * e.T + tap) * e.Cin + ci;
          v = wm[q];
          if (wf) Chunk<T>::store1(wf + q, v);
        }
        tl[r][c] = v;
      }
      __syncthreads();
      if (wd) {
        for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
          const int r = idx >> 6, c = idx & 63;
          const int ci = cib * 64 + r, co = cob * 64 + c;
          if (co < e.Cout && ci < e.Cin)
            Chunk<T>::store1(wd + ((long long)ci * e.T + (e.T - 1 - tap)) * e.Cout + co, tl[c][r]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------ host-side dispatch
#include "hdu_host.h"

int g_tuning[32] = {2, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

extern "C" int hdu_set_tuning(int key, int value) {
  if (key < 0 || key >= 32) return hdu_set_error(HDU_ERR_ARG, "set_tuning: bad key");
  g_tuning[key] = value;
  return 0;
}

// magic numbers of hdu_fastdiv (conv_common.h): exact for dividends below 2^31
static void fastdiv_magic(int d, unsigned* mul, unsigned* shr) {
  if (d <= 1) { *mul = 0u; *shr = 0u; return; }
  int cl = 0;
  while ((1ll << cl) < (long long)d) ++cl;
  const int p = 31 + cl;
  *mul = (unsigned)((((unsigned long long)1 << p) + (unsigned long long)d - 1) / (unsigned long long)d);
  *shr = (unsigned)(p - 32);
}

static int fill_convk(const hdu_conv_desc* d, ConvK* k, bool wgrad, bool exact_grid = false) {
  if (!d) return hdu_set_error(HDU_ERR_ARG, "conv: null descriptor");
  if (d->dtype != HDU_BF16 && d->dtype != HDU_F32) return hdu_set_error(HDU_ERR_ARG, "conv: bad dtype");
  const int ch = d->dtype == HDU_BF16 ? 8 : 4;
  if (d->Cin <= 0 || d->Cin % ch) return hdu_set_error(HDU_ERR_ARG, "conv: Cin must be a positive multiple of the 16-byte chunk");
  if (d->ldx % ch || (d->skip && d->ldskip % ch)) return hdu_set_error(HDU_ERR_ARG, "conv: input pixel stride must be a multiple of the 16-byte chunk");
  if (wgrad && (d->ldy % ch || d->Cout % ch)) return hdu_set_error(HDU_ERR_ARG, "conv_wgrad: dy stride / Cout must be multiples of the 16-byte chunk");
  if ((uintptr_t)d->x % 16 || (uintptr_t)d->w % 16 || (d->skip && (uintptr_t)d->skip % 16))
    return hdu_set_error(HDU_ERR_ARG, "conv: x / w / skip must be 16-byte aligned");
  if ((d->ud | d->uh | d->uw) & ~1) return hdu_set_error(HDU_ERR_ARG, "conv: upsample shifts must be 0 or 1");
  if (d->KD <= 0 || d->KH <= 0 || d->KW <= 0 || d->sd <= 0 || d->sh <= 0 || d->sw <= 0)
    return hdu_set_error(HDU_ERR_ARG, "conv: bad kernel/stride");
  if ((d->pro_a == nullptr) != (d->pro_b == nullptr)) return hdu_set_error(HDU_ERR_ARG, "conv: pro_a/pro_b must both be set");
  k->x = d->x; k->skip = d->skip; k->w = d->w; k->y = d->y;
  k->pro_a = d->pro_a; k->pro_b = d->pro_b; k->bias = d->bias;
  k->epi_a = wgrad ? nullptr : d->epi_a; k->epi_b = d->epi_b; k->epi_relu = d->epi_relu;
  if (k->epi_a && (!k->epi_b || d->accumulate || d->stats_partial || d->bnb_u))
    return hdu_set_error(HDU_ERR_ARG, "conv: the output affine needs epi_b and excludes accumulate / epilogue statistics / the fused BN backward");
  k->ldx = d->ldx; k->ldskip = d->ldskip; k->ldy = d->ldy;
  k->N = d->N; k->Di = d->Di; k->Hi = d->Hi; k->Wi = d->Wi; k->Cin = d->Cin;
  k->ud = d->ud; k->uh = d->uh; k->uw = d->uw;
  k->De = d->Di << d->ud; k->He = d->Hi << d->uh; k->We = d->Wi << d->uw;
  k->KD = d->KD; k->KH = d->KH; k->KW = d->KW;
  k->sd = d->sd; k->sh = d->sh; k->sw = d->sw;
  k->pd = d->pd; k->ph = d->ph; k->pw = d->pw;
  k->Do = d->Do; k->Ho = d->Ho; k->Wo = d->Wo; k->Cout = d->Cout;
  const int eDo = (k->De + 2 * d->pd - d->KD) / d->sd + 1;
  const int eHo = (k->He + 2 * d->ph - d->KH) / d->sh + 1;
  const int eWo = (k->We + 2 * d->pw - d->KW) / d->sw + 1;
  // The kernels test every tap against the input bounds, so an output grid LARGER than the symmetric-padding formula is
  // well defined: the extra positions see implicit zero padding on the high side (the parity classes of a stride-2 data
  // gradient need pad_low = 1, pad_high = 2).  Up to K-1 extra positions per axis are accepted; anything else is an error.
  // The filter-gradient kernels, their plans and the strided gather were written for the exact grid: strict form there.
  const bool exact = wgrad || exact_grid;
  const int xd = exact ? 0 : d->KD - 1, xh = exact ? 0 : d->KH - 1, xw = exact ? 0 : d->KW - 1;
  if (d->Do < eDo || d->Do > eDo + xd || d->Ho < eHo || d->Ho > eHo + xh || d->Wo < eWo || d->Wo > eWo + xw)
    return hdu_set_error(HDU_ERR_ARG, "conv: output dims inconsistent with input dims / kernel / stride / pad");
  k->M = (long long)d->N * d->Do * d->Ho * d->Wo;
  if ((long long)d->N * k->De * k->He * k->We >= (1ll << 31) || k->M >= (1ll << 31))
    return hdu_set_error(HDU_ERR_ARG, "conv: more than 2^31 pixels per tensor (shard the volume)");
  k->Ktot = d->KD * d->KH * d->KW * d->Cin;
  fastdiv_magic(d->Wo, &k->div_wo_mul, &k->div_wo_shr);
  fastdiv_magic(d->Ho, &k->div_ho_mul, &k->div_ho_shr);
  fastdiv_magic(d->Do, &k->div_do_mul, &k->div_do_shr);
  k->spread_h = k->spread_d = 0u;
  if (d->KD * d->KH * d->KW <= 32) {
    for (int q = 0; q < d->KH; ++q) k->spread_h |= 1u << (q * d->KW);
    for (int q = 0; q < d->KD; ++q) k->spread_d |= 1u << (q * d->KH * d->KW);
  }
  fastdiv_magic(d->Cin, &k->div_cin_mul, &k->div_cin_shr);
  fastdiv_magic(d->KW, &k->div_kw_mul, &k->div_kw_shr);
  fastdiv_magic(d->KH, &k->div_kh_mul, &k->div_kh_shr);
  k->sk_div_mul = 0u; k->sk_div_shr = 0u;
  {
    const long long esz = d->dtype == HDU_BF16 ? 2 : 4;
    const long long xb = (((long long)d->N * d->Di * d->Hi * d->Wi - 1) * d->ldx + d->Cin) * esz;
    const long long wb = (long long)d->Cout * k->Ktot * esz;
    k->x_bytes = xb > 0 && xb < (1ll << 32) ? (unsigned)xb : 0u;
    if (g_tuning[HDU_TUNE_DEBUG] & 16) k->x_bytes = 0u;      // tests: take the >= 4 GiB path (64-bit pointers, zero page)
    if (!wgrad && wb >= (1ll << 32)) return hdu_set_error(HDU_ERR_ARG, "conv: filter larger than 4 GiB");
    k->w_bytes = (unsigned)wb;
  }
  k->pro_relu = d->pro_relu; k->accumulate = d->accumulate;
  if (d->drop_keep > 0.f && d->drop_keep < 1.f) {
    k->drop_scale = 1.f / d->drop_keep;
    k->drop_thresh = (unsigned)((double)d->drop_keep * 4294967296.0);
  } else {
    k->drop_scale = 0.f;
    k->drop_thresh = 0xffffffffu;
  }
  k->drop_seed = d->drop_seed;
  k->drop_seed_dev = d->drop_seed_dev;
  k->stats_partial = wgrad ? nullptr : d->stats_partial;
  k->stats_shift = d->stats_shift;
  k->stats_slots = d->stats_slots;
  if (k->stats_partial && (!k->stats_shift || k->stats_slots <= 0 || d->accumulate))
    return hdu_set_error(HDU_ERR_ARG, "conv: epilogue statistics need stats_shift, stats_slots > 0 and accumulate == 0");
  k->bnb_u = wgrad ? nullptr : d->bnb_u; k->bnb_ldu = d->bnb_ldu;
  k->bnb_a = d->bnb_a; k->bnb_b = d->bnb_b; k->bnb_mean = d->bnb_mean; k->bnb_rstd = d->bnb_rstd;
  k->bnb_relu = d->bnb_relu; k->bnb_partial = d->bnb_partial; k->bnb_slots = d->bnb_slots;
  if (k->bnb_u) {
    if (!k->bnb_a || !k->bnb_b || (uintptr_t)k->bnb_u % 16 || k->bnb_ldu % ch || d->pro_a || d->skip || d->bias ||
        d->stats_partial || (d->drop_keep > 0.f && d->drop_keep < 1.f))
      return hdu_set_error(HDU_ERR_ARG, "conv: the fused BN backward needs bnb_a/bnb_b, a 16-byte addressable bnb_u and a plain data-gradient launch (no prologue / skip / bias / dropout / statistics)");
    if (k->bnb_partial && (!k->bnb_mean || !k->bnb_rstd || k->bnb_slots <= 0))
      return hdu_set_error(HDU_ERR_ARG, "conv: bnb_partial needs bnb_mean, bnb_rstd and bnb_slots > 0");
  }
  // the epilogues read the per-channel vectors as 16-byte float4s
  if (((uintptr_t)k->bias | (uintptr_t)k->epi_a | (uintptr_t)k->epi_b | (uintptr_t)(k->stats_partial ? k->stats_shift : nullptr) |
       (uintptr_t)k->bnb_a | (uintptr_t)k->bnb_b | (uintptr_t)k->bnb_mean | (uintptr_t)k->bnb_rstd) & 15)
    return hdu_set_error(HDU_ERR_ARG, "conv: bias / epi_* / stats_shift / bnb_* vectors must be 16-byte aligned");
  k->y_ds = wgrad ? nullptr : d->y_ds; k->ldy_ds = d->ldy_ds;
  k->ds_accumulate = d->ds_accumulate; k->ds_only = d->ds_only;
  if (k->y_ds) {
    if ((d->Ho | d->Wo) & 1) return hdu_set_error(HDU_ERR_ARG, "conv: the down-sampled output needs even Ho and Wo");
    if ((uintptr_t)k->y_ds % 16 || k->ldy_ds % ch || k->ldy_ds < d->Cout)
      return hdu_set_error(HDU_ERR_ARG, "conv: y_ds must be 16-byte aligned and ldy_ds a multiple of the 16-byte chunk >= Cout");
    if (d->accumulate) return hdu_set_error(HDU_ERR_ARG, "conv: the down-sampled output excludes accumulate (it sums what a plain store holds)");
    if (exact_grid) return hdu_set_error(HDU_ERR_ARG, "conv: the down-sampled output is a halo-wide hdu_conv_fprop epilogue only");
  } else if (!wgrad && (d->ds_only || d->ds_accumulate)) {
    return hdu_set_error(HDU_ERR_ARG, "conv: ds_only / ds_accumulate without y_ds");
  }
  k->M_layer = d->layer_rows > 0 ? d->layer_rows : k->M;
  k->sk_ws = wgrad ? nullptr : (float*)d->splitk_ws;
  k->sk_cnt = wgrad ? nullptr : d->splitk_counters;
  if (k->sk_ws && ((uintptr_t)k->sk_ws % 16 || !k->sk_cnt))
    return hdu_set_error(HDU_ERR_ARG, "conv: splitk_ws must be 16-byte aligned and come with splitk_counters");
  k->xcd_swizzle = g_tuning[HDU_TUNE_XCD_SWIZZLE];
  k->vec_out = 1;
  k->debug_flags = g_tuning[HDU_TUNE_DEBUG];
  k->f32_split = (d->dtype == HDU_F32 && g_tuning[HDU_TUNE_F32_SPLIT]) ? 1 : 0;
  if (!wgrad && d->y && (d->Cout % ch || d->ldy % ch || (uintptr_t)d->y % 16))
    return hdu_set_error(HDU_ERR_ARG, "conv: Cout / output pixel stride must be multiples of the 16-byte chunk and y 16-byte aligned");
  return 0;
}

// FAST addressing needs: no up-sampling, <= 32 taps, every element offset of the input within int32
static bool igemm_fast_ok(const ConvK& k) {
  if (g_tuning[HDU_TUNE_NO_FAST]) return false;
  if ((k.ud | k.uh | k.uw) != 0 || k.KD * k.KH * k.KW > 32) return false;
  const long long span = ((long long)k.N * k.De * k.He * k.We + (long long)k.He * k.We * 8) * k.ldx;
  return span < (1ll << 31) && k.x_bytes != 0;     // (x_bytes == 0: the tensor does not fit a 32-bit byte offset)
}

static bool conv_pointwise(const ConvK& k) {
  return k.KD * k.KH * k.KW == 1 && k.sd == 1 && k.sh == 1 && k.sw == 1 && (k.pd | k.ph | k.pw) == 0 && (k.ud | k.uh | k.uw) == 0;
}

// the BN(+Scale)+ReLU prologue of a pointwise conv runs on the async-DMA kernels (PRO instantiations): FAST addressing
// (tensor < 2^31 elements / 4 GiB), the whole a / b range in the LDS table, plain output grid
static bool igemm_pro_dma_ok(const ConvK& k) {
  return k.pro_a != nullptr && k.skip == nullptr && k.vec_out && k.bnb_u == nullptr && conv_pointwise(k) && k.Cin <= HDU_PRO_CMAX &&
         k.Do == k.De && k.Ho == k.He && k.Wo == k.We && igemm_fast_ok(k) && !g_tuning[HDU_TUNE_NO_PRO_DMA] &&
         ((uintptr_t)k.pro_a % 16 == 0) && ((uintptr_t)k.pro_b % 16 == 0);
}

// Split-K factor of a small-grid launch (ring kernel).  A grid of <= 128 workgroups leaves half the chip idle and each
// busy compute unit is bound by what it alone can pull from L2 (measured: 14-20 KB per K step at ~1 us per step whatever
// the MFMA work), so the K steps are dealt to S workgroups per tile until ~256 workgroups run, keeping >= 4 K steps per
// split and S <= 16 (the last arriver reads S-1 partial tiles).  `bytes`: scratch the launch needs.
// bf16 64-row tiles run a 3-stage ring (<= 72 KB of LDS): two workgroups share a CU, so a split launch aims at 512
static int ring_wgs_per_cu(int bm, bool bf16) { return (bm == 64 && bf16) ? 2 : 1; }

static int choose_splitk(long long nblk, int nk, int bm, int bn, int per_cu, size_t* bytes) {
  *bytes = 0;
  const int mode = g_tuning[HDU_TUNE_SPLITK];
  const int target = g_tuning[HDU_TUNE_SPLITK_TARGET] > 0 ? g_tuning[HDU_TUNE_SPLITK_TARGET] : 256 * per_cu;
  const int min_steps = g_tuning[HDU_TUNE_SPLITK_MIN_STEPS] > 0 ? g_tuning[HDU_TUNE_SPLITK_MIN_STEPS] : 4;   // swept: profiles/r02_experiment_splitk_sweep.txt
  if (mode == 1 || nblk > target / 2) return 1;
  int S = mode >= 2 ? mode : (int)((target + nblk - 1) / nblk);
  if (S > nk / min_steps) S = nk / min_steps;
  if (S > 16) S = 16;
  if (S < 2) return 1;
  *bytes = (size_t)nblk * (size_t)S * (size_t)bm * (size_t)bn * sizeof(float);
  return S;
}

static bool igemm_ring_ok(long long nblk, int Ktot, int stage_bytes, int nsd) {
  const int mode = g_tuning[HDU_TUNE_DMA_STAGES];
  return stage_bytes * nsd <= 160 * 1024 && (mode == 6 || (mode == 2 && nblk <= 256 && Ktot > g_tuning[HDU_TUNE_RING_MIN_K]));
}

// ring depth of a PRO launch: the a / b table rides on top of the operand stages, stages are dropped until it fits
template <typename T, int BM, int BN, int PROC> struct ProRing {
  static constexpr int STAGE = (BM + ((BN + 31) / 32) * 32) * 128;
  static constexpr int NSD = STAGE * 6 <= 160 * 1024 ? 6 : 4;
  static constexpr int NSR0 = (BM == 64 && sizeof(T) == 2 && NSD == 6) ? 3 : NSD;
  static constexpr int NSR = (NSR0 * STAGE + 8 * PROC <= 160 * 1024) ? NSR0 : (NSR0 == 6 ? 4 : 3);
  static_assert(NSR * STAGE + 8 * PROC <= 160 * 1024, "LDS");
};

template <typename T, int BM, int BN, int WMv, int WNv, int PROC>
static void launch_igemm_pro(const ConvK& k, dim3 grid, size_t sk_bytes_avail, hipStream_t s) {
  typedef ProRing<T, BM, BN, PROC> R;
  const long long nblk = (long long)grid.x * grid.y;
  const long long nblk_layer = (long long)((k.M_layer + BM - 1) / BM) * grid.y;
  if (igemm_ring_ok(nblk_layer, k.Ktot, R::STAGE, R::NSD)) {
    constexpr int BK = 8 * Chunk<T>::CH;
    size_t need;
    const int S = choose_splitk(nblk_layer, (k.Ktot + BK - 1) / BK, BM, BN, ring_wgs_per_cu(BM, sizeof(T) == 2), &need);
    need = need / (size_t)nblk_layer * (size_t)nblk;
    ConvK kk = k;
    if (S > 1 && k.sk_ws && k.sk_cnt && need <= sk_bytes_avail && nblk <= 512) {
      grid.z = (unsigned)S;
      fastdiv_magic(S, &kk.sk_div_mul, &kk.sk_div_shr);
    }
    HDU_LAUNCH((conv_igemm_ring_kernel<T, BM, BN, WMv, WNv, R::NSR, true, false, PROC>), grid, dim3(256), 0, s, kk);
  } else {
    HDU_LAUNCH((conv_igemm_dma_kernel<T, BM, BN, WMv, WNv, true, false, PROC>), grid, dim3(256), 0, s, k);
  }
}

template <typename T, int BM, int BN, int WMv, int WNv>
static void launch_igemm(const ConvK& k, size_t sk_bytes_avail, hipStream_t s) {
  dim3 grid((unsigned)((k.M + BM - 1) / BM), (unsigned)((k.Cout + BN - 1) / BN), 1);
  if (igemm_pro_dma_ok(k)) {
    // pointwise conv over relu(a * x + b): the DMA kernels with the affine applied to the A fragment in registers (PRO)
    if (k.Cin <= HDU_PRO_CSMALL) launch_igemm_pro<T, BM, BN, WMv, WNv, HDU_PRO_CSMALL>(k, grid, sk_bytes_avail, s);
    else launch_igemm_pro<T, BM, BN, WMv, WNv, HDU_PRO_CMAX>(k, grid, sk_bytes_avail, s);
    return;
  }
  if (k.pro_a == nullptr && k.skip == nullptr && k.vec_out) {
    // deep ring when the grid cannot fill the chip (latency-bound K loop, LDS is free); else 2 stages x 3 blocks/CU
    constexpr int STAGE = (BM + ((BN + 31) / 32) * 32) * 128;
    constexpr int NSD = STAGE * 6 <= 160 * 1024 ? 6 : 4;
    const long long nblk = (long long)grid.x * grid.y;
    const long long nblk_layer = (long long)((k.M_layer + BM - 1) / BM) * grid.y;     // the whole (unsharded) layer's grid
    const int mode = g_tuning[HDU_TUNE_DMA_STAGES];
    const bool fast = igemm_fast_ok(k);
    if (igemm_ring_ok(nblk_layer, k.Ktot, STAGE, NSD)) {
      constexpr int BK = 8 * Chunk<T>::CH;
      size_t need;
      const int S = choose_splitk(nblk_layer, (k.Ktot + BK - 1) / BK, BM, BN, ring_wgs_per_cu(BM, sizeof(T) == 2), &need);
      need = need / (size_t)nblk_layer * (size_t)nblk;                  // scratch for THIS launch's tiles
      ConvK kk = k;
      if (S > 1 && k.sk_ws && k.sk_cnt && need <= sk_bytes_avail && nblk <= 512) {      // (512 ticket counters)
        grid.z = (unsigned)S;
        fastdiv_magic(S, &kk.sk_div_mul, &kk.sk_div_shr);
      }
      // 64-row bf16 tiles: THREE stages (<= 72 KB) so that two workgroups share a CU and the prologue issues 2 tiles,
      // not 5, before the first MFMA (measured r02 calls P / Q against the 6-stage ring: 3dpart 11.09 -> 10.70 ms with
      // the 512-workgroup split target, end2end 17.23 -> 16.81, 2D 21.62 -> 21.57; 4 stages in between)
      constexpr int NSR = (BM == 64 && sizeof(T) == 2 && NSD == 6) ? 3 : NSD;
      // (the fused BN backward rides on FAST-addressed launches: a data gradient has no up-sampling and <= 27 taps; a
      // descriptor that is not FAST takes the late-load epilogue of the plain instantiation's BNB twin below)
      if (k.bnb_u != nullptr) {
        if (fast) HDU_LAUNCH((conv_igemm_ring_kernel<T, BM, BN, WMv, WNv, NSR, true, true>), grid, dim3(256), 0, s, kk);
        else HDU_LAUNCH((conv_igemm_ring_kernel<T, BM, BN, WMv, WNv, NSR, false, true>), grid, dim3(256), 0, s, kk);
      } else if (fast) HDU_LAUNCH((conv_igemm_ring_kernel<T, BM, BN, WMv, WNv, NSR, true>), grid, dim3(256), 0, s, kk);
      else HDU_LAUNCH((conv_igemm_ring_kernel<T, BM, BN, WMv, WNv, NSR, false>), grid, dim3(256), 0, s, kk);
    } else {
      if (k.bnb_u != nullptr) {
        if (fast) HDU_LAUNCH((conv_igemm_dma_kernel<T, BM, BN, WMv, WNv, true, true>), grid, dim3(256), 0, s, k);
        else HDU_LAUNCH((conv_igemm_dma_kernel<T, BM, BN, WMv, WNv, false, true>), grid, dim3(256), 0, s, k);
      } else if (fast) HDU_LAUNCH((conv_igemm_dma_kernel<T, BM, BN, WMv, WNv, true>), grid, dim3(256), 0, s, k);
      else HDU_LAUNCH((conv_igemm_dma_kernel<T, BM, BN, WMv, WNv, false>), grid, dim3(256), 0, s, k);
    }
  } else
    HDU_LAUNCH((conv_igemm_kernel<T, BM, BN, WMv, WNv>), grid, dim3(256), 0, s, k);
}

// tile choice.  Every N tile re-loads the whole A operand (the activations), and for Cout <= 192 a single N tile also
// writes full output rows, so wide tiles are preferred: cost model = n_tiles * (BN + 32) (MFMA columns + the A-load
// expressed in column equivalents); 64-row tiles below 16 K pixels.
static void choose_igemm(const ConvK& k, int* bm, int* bn) {
  // 192-column tiles (one N tile for the 192-channel bottleneck outputs / 3x3 data gradients: 29 % fewer DMA instructions
  // per FLOP, still 2 workgroups / CU) were measured slower in both rounds (r02: 2D 21.6 -> 22.0 ms, 3dpart 11.09 -> 11.17,
  // profiles/r02_experiment_knob_probes.txt); their f32 form cannot be staged in the operand LDS anyway.
  const int cands[5] = {128, 96, 64, 48, 32};
  int best = 64;
  long long best_cost = -1;
  const int maxbn = g_tuning[HDU_TUNE_MAX_BN] > 0 ? g_tuning[HDU_TUNE_MAX_BN] : 128;
  for (int i = 0; i < 5; ++i) {
    const int c = cands[i];
    if (c > maxbn) continue;
    const long long ntiles = (k.Cout + c - 1) / c;
    const long long cost = ntiles * (c + 32);
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = c; }
  }
  *bn = best;
  *bm = (k.M_layer <= (g_tuning[HDU_TUNE_BM64_MAX_M] > 0 ? (long long)g_tuning[HDU_TUNE_BM64_MAX_M] : 16384)) ? 64 : 128;
}

template <int BM, int BN> struct WaveLayout {           // (waves along M, waves along N)
  static constexpr int WM = (BN >= 128) ? 2 : ((BM == 64 && (BN == 64 || BN == 32)) ? 2 : 4);
  static constexpr int WN = 4 / WM;
};

template <typename T, int BM>
static void dispatch_igemm_bn(const ConvK& k, int bn, size_t skb, hipStream_t s) {
  switch (bn) {
    case 128: launch_igemm<T, BM, 128, WaveLayout<BM, 128>::WM, WaveLayout<BM, 128>::WN>(k, skb, s); return;
    case 96: launch_igemm<T, BM, 96, WaveLayout<BM, 96>::WM, WaveLayout<BM, 96>::WN>(k, skb, s); return;
    case 64: launch_igemm<T, BM, 64, WaveLayout<BM, 64>::WM, WaveLayout<BM, 64>::WN>(k, skb, s); return;
    case 48: launch_igemm<T, BM, 48, WaveLayout<BM, 48>::WM, WaveLayout<BM, 48>::WN>(k, skb, s); return;
    default: launch_igemm<T, BM, 32, WaveLayout<BM, 32>::WM, WaveLayout<BM, 32>::WN>(k, skb, s); return;
  }
}

// persistent 256-row form (conv_igemm_pers_kernel): plain or pointwise-with-BN-prologue launches on FAST addressing whose
// (m-tile, n-tile) list gives every one of the CU-resident workgroups at least `HDU_TUNE_PERS_MIN_ITEMS` / CUs tiles
static int pers_table_cap(int bn, int cin) {                 // LDS table capacity for the prologue, -1 = does not fit
  const int stage3 = 3 * (256 + bn) * 128;
  if (cin <= HDU_PRO_CSMALL && stage3 + 8 * HDU_PRO_CSMALL <= 160 * 1024) return HDU_PRO_CSMALL;
  if (stage3 + 8 * HDU_PRO_CMAX <= 160 * 1024) return HDU_PRO_CMAX;
  return -1;
}

static bool igemm_pers_ok(const ConvK& k, int bn) {
  if (g_tuning[HDU_TUNE_PERS] == 0) return false;
  if (k.skip != nullptr || !k.vec_out || k.bnb_u != nullptr || !igemm_fast_ok(k)) return false;
  if (k.f32_split) return false;      // (the persistent body contracts in the exact form only: a split-bf16 net must not mix the two by grid size -- ADVICE r4)
  if (k.pro_a != nullptr && (!igemm_pro_dma_ok(k) || pers_table_cap(bn, k.Cin) < 0)) return false;
  const long long items = ((k.M_layer + 255) / 256) * ((k.Cout + bn - 1) / bn);
  const int min_items = g_tuning[HDU_TUNE_PERS_MIN_ITEMS] > 0 ? g_tuning[HDU_TUNE_PERS_MIN_ITEMS] : 512;
  return items >= min_items && k.M < (1ll << 31) - 256;
}

template <typename T, int BN>
static void launch_pers(const ConvK& k, hipStream_t s) {
  const int tiles_m = (int)((k.M + 255) / 256), tiles_n = (k.Cout + BN - 1) / BN;
  const int cus = g_tuning[HDU_TUNE_PERS] > 1 ? g_tuning[HDU_TUNE_PERS] : 256;        // one workgroup per CU (MI355X: 256)
  long long items = (long long)tiles_m * tiles_n;
  const dim3 grid((unsigned)(items < cus ? items : cus));
  if (k.pro_a != nullptr) {
    const int cap = pers_table_cap(BN, k.Cin);
    if (cap == HDU_PRO_CSMALL) {
      if constexpr (3 * (256 + BN) * 128 + 8 * HDU_PRO_CSMALL <= 160 * 1024)
        HDU_LAUNCH((conv_igemm_pers_kernel<T, BN, HDU_PRO_CSMALL>), grid, dim3(512), 0, s, k, tiles_m, tiles_n);
    } else {
      if constexpr (3 * (256 + BN) * 128 + 8 * HDU_PRO_CMAX <= 160 * 1024)
        HDU_LAUNCH((conv_igemm_pers_kernel<T, BN, HDU_PRO_CMAX>), grid, dim3(512), 0, s, k, tiles_m, tiles_n);
    }
  } else {
    HDU_LAUNCH((conv_igemm_pers_kernel<T, BN, 0>), grid, dim3(512), 0, s, k, tiles_m, tiles_n);
  }
}

template <typename T>
static void dispatch_igemm(const ConvK& k, size_t skb, hipStream_t s) {
  int bm, bn;
  choose_igemm(k, &bm, &bn);
  if (bm == 128 && igemm_pers_ok(k, bn)) {
    switch (bn) {
      case 128: launch_pers<T, 128>(k, s); return;
      case 96: launch_pers<T, 96>(k, s); return;
      case 64: launch_pers<T, 64>(k, s); return;
      case 48: launch_pers<T, 48>(k, s); return;
      default: launch_pers<T, 32>(k, s); return;
    }
  }
  if (bm == 64) dispatch_igemm_bn<T, 64>(k, bn, skb, s);
  else dispatch_igemm_bn<T, 128>(k, bn, skb, s);
}

// conv_halo_wide.hip: halo-tile kernel for the wide 3x3 / 3x3x3 layers (round 5)
bool hdu_halo_wide_taken(const ConvK& k, int dtype);
const char* hdu_halo_wide_name(const ConvK& k, int dtype);
bool hdu_halo_wide_launch(const ConvK& k, int dtype, hipStream_t s);
bool hdu_stem_wgrad_taken(const ConvK& k, int dtype);
bool hdu_stem_wgrad_launch(const ConvK& k, int dtype, float* dw, hipStream_t s);

static bool fprop_halo_ok(const ConvK& k, int dtype) {
  return dtype == HDU_BF16 && k.bnb_u == nullptr && !g_tuning[HDU_TUNE_NO_HALO_FPROP] && k.pro_a == nullptr && k.skip == nullptr && k.KD == 1 &&
         k.KH == 3 && k.KW == 3 && k.sd == 1 && k.sh == 1 && k.sw == 1 && k.pd == 0 && k.ph == 1 && k.pw == 1 &&
         (k.ud | k.uh | k.uw) == 0 && k.Di == 1 && k.Cin % 8 == 0 && k.We >= 32 && k.He >= 4 &&
         // the kernel addresses its output with the INPUT grid (3x3, pad 1: equal); an enlarged output grid (fill_convk
         // accepts up to K-1 extra positions for the parity classes of a stride-2 data gradient) goes to the im2col path
         k.Do == 1 && k.Ho == k.He && k.Wo == k.We &&
         // measured: pays when the K loop is long (>= 4 chunks of 32 channels) and one N tile covers Cout
         k.Cin >= 128 && k.Cout <= 96 &&
         // ... and when its 4x32-pixel tiles fill the chip: below that the im2col ring kernel with split-K spreads the
         // layer over more compute units (each halo workgroup has to pull the whole 9-tap filter tile)
         // (a depth shard decides for the whole layer, like the split-K count: hdu_conv_desc.layer_rows)
         (long long)k.N * ((k.He + 3) / 4) * ((k.We + 31) / 32) * k.M_layer / k.M >= (g_tuning[HDU_TUNE_HALO_MIN_TILES] > 0 ? g_tuning[HDU_TUNE_HALO_MIN_TILES] : 128);
}

static int choose_halo_bn(const ConvK& k) {
  const int cands[4] = {96, 64, 48, 32};     // 128 would need 174 KB of LDS for the two stages
  int best = 64;
  long long best_cost = -1;
  for (int i = 0; i < 4; ++i) {
    const int c = cands[i];
    const long long cost = (long long)((k.Cout + c - 1) / c) * (c + 24);
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = c; }
  }
  return best;
}

template <int BN>
static void launch_halo_fprop(const ConvK& k, hipStream_t s) {
  const unsigned tiles = (unsigned)(k.N * ((k.He + 3) / 4) * ((k.We + 31) / 32));
  HDU_LAUNCH((conv_halo_fprop_kernel<BN>), dim3(tiles, (unsigned)((k.Cout + BN - 1) / BN)), dim3(256), 0, s, k);
}

// filter-stationary streaming form (conv_pw_bstat_kernel): plain pointwise launches with a 2- or 3-step contraction and at
// least two 128-channel output groups -- the bottleneck data gradients
static bool pw_bstat_ok(const ConvK& k, int dtype) {
  return dtype == HDU_BF16 && !g_tuning[HDU_TUNE_NO_PW_BSTAT] && k.KD * k.KH * k.KW == 1 && k.sd == 1 && k.sh == 1 && k.sw == 1 &&
         (k.pd | k.ph | k.pw) == 0 && (k.ud | k.uh | k.uw) == 0 && k.pro_a == nullptr && k.skip == nullptr && k.bias == nullptr &&
         k.epi_a == nullptr && k.stats_partial == nullptr && (k.bnb_u != nullptr ? (!g_tuning[HDU_TUNE_NO_PW_BSTAT_BNB] && !(k.bnb_relu & 6)) : !k.accumulate) &&
         k.drop_scale == 0.f &&
         (k.Ktot == 128 || k.Ktot == 192) && k.Cout >= 256 && k.M >= 64 && k.x_bytes != 0 &&
         // (round 6: the output / BN-input chunks travel through raw buffer resources with 32-bit byte offsets)
         (k.M - 1) * k.ldy + k.Cout < (1ll << 31) && (k.bnb_u == nullptr || (k.M - 1) * k.bnb_ldu + k.Cout < (1ll << 31)) &&
         (long long)k.Cout * k.Ktot * 2 < (1ll << 31) && k.Do == k.De && k.Ho == k.He && k.Wo == k.We;
}

// Two forms.  128 output channels per workgroup, three-slot operand ring (138 KB of LDS: ONE workgroup per CU), and -- round 6 --
// 64 channels, two slots, exactly 80 KB: TWO workgroups per CU.  tools/bench_pw_bstat.py showed the kernel bound per CU, not
// by memory: 64 / 128 / 256 workgroups of the one-per-CU form take 36 / 20 / 13 us on the same launch (a single 4-wave workgroup pulls
// ~10 B/clk through its CU whatever its prefetch depth -- DESIGN.md section 3.1's streaming micro-benchmark), so the lever is waves per CU.
// HDU_TUNE_PW_BSTAT_FORM: 0 = chosen here, 1 = always the 128-channel form, 2 = always the 64-channel form.
template <int BN, int NSA>
static void launch_pw_bstat_form(const ConvK& k, int target, hipStream_t s) {
  const unsigned ny = (unsigned)((k.Cout + BN - 1) / BN);
  long long splits = target / (long long)ny;
  if (splits < 1) splits = 1;
  const long long tiles = (k.M + 63) / 64;
  if (splits > tiles) splits = tiles;
  const long long rows = ((tiles + splits - 1) / splits) * 64;
  const unsigned gx = (unsigned)((k.M + rows - 1) / rows);
  if (k.bnb_u != nullptr) {
    if (k.Ktot == 192) HDU_LAUNCH((conv_pw_bstat_kernel<3, BN, true, NSA>), dim3(gx, ny), dim3(256), 0, s, k, (int)rows);
    else HDU_LAUNCH((conv_pw_bstat_kernel<2, BN, true, NSA>), dim3(gx, ny), dim3(256), 0, s, k, (int)rows);
    return;
  }
  if (k.Ktot == 192) HDU_LAUNCH((conv_pw_bstat_kernel<3, BN, false, NSA>), dim3(gx, ny), dim3(256), 0, s, k, (int)rows);
  else HDU_LAUNCH((conv_pw_bstat_kernel<2, BN, false, NSA>), dim3(gx, ny), dim3(256), 0, s, k, (int)rows);
}

static int pw_bstat_form(const ConvK& k) {
  const int f = g_tuning[HDU_TUNE_PW_BSTAT_FORM];
  if (f == 1 || f == 2) return f;
  // measured per shape with the XCD-major workgroup order (tools/bench_pw_bstat.py, profiles/r06_experiment_pw_bstat_forms.txt; us per
  // launch, form 1 / form 2; round 5's kernel in brackets): BN-backward form M = 2048: 12.4 / 10.9 [12.0]; M = 8192, C = 1584:
  // 28.4 / 24.9 [29.3]; C = 624: 15.5 / 13.7 [17.2]; M = 32768: 35.7 / 28.9 [39.8].  Plain form (store only): 5.8 / 6.2, 13.1 / 15.5,
  // 17.2 / 19.1 -- its tile is one operand DMA and one store, the doubled operand traffic of the 64-channel form is not paid back.
  return k.bnb_u != nullptr ? 2 : 1;
}

static void launch_pw_bstat(const ConvK& k, hipStream_t s) {
  const int wgs = g_tuning[HDU_TUNE_PW_BSTAT_WGS];
  if (pw_bstat_form(k) == 2) launch_pw_bstat_form<64, 2>(k, wgs > 0 ? wgs : 512, s);
  else launch_pw_bstat_form<128, 3>(k, wgs > 0 ? wgs : 256, s);
}

extern "C" int hdu_conv_fprop(const hdu_conv_desc* d, void* stream) {
  ConvK k;
  if (int e = fill_convk(d, &k, false)) return e;
  if (!d->y) return hdu_set_error(HDU_ERR_ARG, "conv_fprop: null output");
  if (k.M == 0) return 0;
  if (k.y_ds && !hdu_halo_wide_taken(k, d->dtype))      // (only the halo-wide epilogue forms it: never a silently missing output)
    return hdu_set_error(HDU_ERR_ARG, "conv_fprop: y_ds needs a launch that a halo-wide configuration takes");
  if (pw_bstat_ok(k, d->dtype)) {
    launch_pw_bstat(k, (hipStream_t)stream);
    return hdu_check_launch("conv_fprop(pointwise, filter-stationary)");
  }
  if (hdu_halo_wide_launch(k, d->dtype, (hipStream_t)stream)) return hdu_check_launch("conv_fprop(halo, wide)");
  if (fprop_halo_ok(k, d->dtype)) {
    switch (choose_halo_bn(k)) {
      case 96: launch_halo_fprop<96>(k, (hipStream_t)stream); break;
      case 64: launch_halo_fprop<64>(k, (hipStream_t)stream); break;
      case 48: launch_halo_fprop<48>(k, (hipStream_t)stream); break;
      default: launch_halo_fprop<32>(k, (hipStream_t)stream); break;
    }
    return hdu_check_launch("conv_fprop(halo)");
  }
  if (d->dtype == HDU_BF16) dispatch_igemm<bf16_t>(k, d->splitk_ws_bytes, (hipStream_t)stream);
  else dispatch_igemm<float>(k, d->splitk_ws_bytes, (hipStream_t)stream);
  return hdu_check_launch("conv_fprop");
}

extern "C" size_t hdu_conv_splitk_ws_bytes(const hdu_conv_desc* d) {
  ConvK k;
  if (fill_convk(d, &k, false)) return 0;
  if (k.M == 0 || pw_bstat_ok(k, d->dtype) || hdu_halo_wide_taken(k, d->dtype) || fprop_halo_ok(k, d->dtype) || (k.pro_a != nullptr && !igemm_pro_dma_ok(k)) || k.skip != nullptr) return 0;
  int bm, bn;
  choose_igemm(k, &bm, &bn);
  if (bm == 128 && igemm_pers_ok(k, bn)) return 0;
  const long long nblk = ((k.M + bm - 1) / bm) * ((k.Cout + bn - 1) / bn);
  const long long nblk_layer = ((k.M_layer + bm - 1) / bm) * ((k.Cout + bn - 1) / bn);
  const int stage = (bm + ((bn + 31) / 32) * 32) * 128;
  const int nsd = stage * 6 <= 160 * 1024 ? 6 : 4;
  if (!igemm_ring_ok(nblk_layer, k.Ktot, stage, nsd)) return 0;
  const int bk = d->dtype == HDU_BF16 ? 64 : 32;
  size_t need;
  choose_splitk(nblk_layer, (k.Ktot + bk - 1) / bk, bm, bn, ring_wgs_per_cu(bm, d->dtype == HDU_BF16), &need);
  return need / (size_t)nblk_layer * (size_t)nblk;
}

template <typename T, int BCO>
static void launch_wgrad(const ConvK& k, float* dw, hipStream_t s) {
  constexpr int PX = 8 * Chunk<T>::CH;
  const unsigned gx = (unsigned)((k.Ktot + 127) / 128), gy = (unsigned)((k.Cout + BCO - 1) / BCO);
  // enough pixel splits to fill the chip (~4 workgroups per CU), each a multiple of the pixel step.  HDU_TUNE_WGRAD_TARGET_WGS = 1
  // gives ONE split per tile: every dw element then has a single writer and the launch is bit-reproducible (the float atomics of
  // several splits arrive in any order) -- the "ordered reductions" recipe of the parity tests' weight training (tests/parity_utils.py)
  const long long target = g_tuning[HDU_TUNE_WGRAD_TARGET_WGS] > 0 ? g_tuning[HDU_TUNE_WGRAD_TARGET_WGS] : 1024;
  long long want = target / ((long long)gx * gy);
  if (want < 1) want = 1;
  long long steps = (k.M + PX - 1) / PX;
  if (want > steps) want = steps;
  long long steps_per = (steps + want - 1) / want;
  const long long rows_per = steps_per * PX;
  const unsigned gz = (unsigned)((k.M + rows_per - 1) / rows_per);
  HDU_LAUNCH((conv_wgrad_kernel<T, BCO>), dim3(gx, gy, gz), dim3(256), 0, s, k, dw, rows_per);
}

static int choose_wgrad(const ConvK& k) {
  const int cands[3] = {64, 48, 32};
  int best = 64;
  long long best_cost = -1;
  for (int i = 0; i < 3; ++i) {
    const long long padded = (long long)((k.Cout + cands[i] - 1) / cands[i]) * cands[i];
    if (best_cost < 0 || padded < best_cost) { best_cost = padded; best = cands[i]; }
  }
  return best;
}

// 1-D grid of the filter-gradient kernels (wgrad_block in conv_common.h)
static unsigned wgrad_grid(const ConvK& k) { return (unsigned)k.wg_gz * (unsigned)(k.wg_gx * k.wg_gy); }


static bool wgrad_pointwise(const ConvK& k) {
  return k.KD * k.KH * k.KW == 1 && k.sd == 1 && k.sh == 1 && k.sw == 1 && (k.pd | k.ph | k.pw) == 0 &&
         (k.ud | k.uh | k.uw) == 0;
}

// work grid of the DMA filter gradient: k-column tiles x filter-row tiles x pixel splits.  Pixel splits: fill the chip
// (`target` workgroups) but keep >= min_steps steps of 64 pixels per workgroup so that the pipeline fill and the float
// atomics of the partial tile are amortised.  Returns the pixel rows per split.
// filter-row tiles one workgroup accumulates (wgrad_dma_body NCT): pointwise layers whose Cout spans 2 or 3 tiles of 64
static int wgrad_nct(const ConvK& k, int BCO) {
  if (g_tuning[HDU_TUNE_WGRAD_NCT] == 1 || !wgrad_pointwise(k) || BCO != 64) return 1;
  const int tiles = (k.Cout + BCO - 1) / BCO;
  return tiles >= 3 ? 3 : (tiles == 2 ? 2 : 1);
}

// the DMA filter-gradient kernels take operands that need no arithmetic -- or, for POINTWISE layers, the producer's
// BN(+Scale)+ReLU as two per-lane scalars on the transposed x fragment (wgrad_dma_body)
static bool wgrad_dma_ok(const ConvK& k) {
  return k.skip == nullptr && (k.pro_a == nullptr || (wgrad_pointwise(k) && !g_tuning[HDU_TUNE_NO_PRO_DMA]));
}

static long long wgrad_dma_geometry(const ConvK& k, int BCO, int target, ConvK* kk, int default_min_steps = 4, int nct = 1) {
  constexpr int PX = 64;
  const unsigned gx = (unsigned)((k.Ktot + 127) / 128), gy = (unsigned)((k.Cout + BCO * nct - 1) / (BCO * nct));
  long long want = target / ((long long)gx * gy);
  if (want < 1) want = 1;
  long long steps = (k.M + PX - 1) / PX;
  const int min_steps = g_tuning[HDU_TUNE_WGRAD_MIN_STEPS] > 0 ? g_tuning[HDU_TUNE_WGRAD_MIN_STEPS] : default_min_steps;
  if (want > (steps + min_steps - 1) / min_steps) want = (steps + min_steps - 1) / min_steps;
  if (want < 1) want = 1;
  long long steps_per = (steps + want - 1) / want;
  const long long rows_per = steps_per * PX;
  const unsigned gz = (unsigned)((k.M + rows_per - 1) / rows_per);
  *kk = k;
  kk->wg_gx = (int)gx; kk->wg_gy = (int)gy; kk->wg_gz = (int)gz;
  return rows_per;
}

template <int BCO>
static void launch_wgrad_tr(const ConvK& k, float* dw, hipStream_t s) {
  const int target = g_tuning[HDU_TUNE_WGRAD_TARGET_WGS] > 0 ? g_tuning[HDU_TUNE_WGRAD_TARGET_WGS] : 768;
  ConvK kk;
  const bool dma = wgrad_dma_ok(k);
  const int nct = dma ? wgrad_nct(k, BCO) : 1;
  const long long rows_per = wgrad_dma_geometry(k, BCO, target, &kk, 4, nct);
  if (dma) {
    if constexpr (BCO == 64) {
      if (nct == 3) { HDU_LAUNCH((conv_wgrad_dma_kernel<64, true, 3>), dim3(wgrad_grid(kk)), dim3(256), 0, s, kk, dw, rows_per); return; }
      if (nct == 2) { HDU_LAUNCH((conv_wgrad_dma_kernel<64, true, 2>), dim3(wgrad_grid(kk)), dim3(256), 0, s, kk, dw, rows_per); return; }
    }
    if (wgrad_pointwise(k)) HDU_LAUNCH((conv_wgrad_dma_kernel<BCO, true>), dim3(wgrad_grid(kk)), dim3(256), 0, s, kk, dw, rows_per);
    else HDU_LAUNCH((conv_wgrad_dma_kernel<BCO, false>), dim3(wgrad_grid(kk)), dim3(256), 0, s, kk, dw, rows_per);
  } else
    HDU_LAUNCH((conv_wgrad_tr_kernel<BCO>), dim3((unsigned)kk.wg_gx, (unsigned)kk.wg_gy, (unsigned)kk.wg_gz), dim3(256), 0, s,
               k, dw, rows_per);
}

static bool wgrad_halo_ok(const ConvK& k) {
  // 2D 3 x 3 "same" layers, and (round 4, HDU_TUNE_NO_HALO bit 1 = off) 3 x 3 x 3 "same" layers as three plane-shifted 2D problems
  const bool d2 = k.KD == 1 && k.pd == 0 && k.Di == 1;
  // depth: "same" (pd 1), "valid" over stored halo planes (pd 0: the depth-sharded layers), or valid behind a depth up-sampling of
  // the stored halo planes (pd -1: their decoder) -- input plane = output plane + kd - pd in every case
  const bool d3 = k.KD == 3 && k.pd >= -1 && k.pd <= 1 && k.Do == k.De + 2 * k.pd - 2 && k.Ho == k.He && k.Wo == k.We &&
                  !(g_tuning[HDU_TUNE_NO_HALO] & 2);
  return !(g_tuning[HDU_TUNE_NO_HALO] & 1) && k.pro_a == nullptr && k.skip == nullptr && (d2 || d3) && k.KH == 3 && k.KW == 3 &&
         k.sd == 1 && k.sh == 1 && k.sw == 1 && k.ph == 1 && k.pw == 1 &&
         // (a nearest-neighbour up-sampling in front of the conv is resolved in the tile's addressing: bit 2 of the knob = off)
         ((k.ud | k.uh | k.uw) == 0 || !(g_tuning[HDU_TUNE_NO_HALO] & 4)) &&
         k.Cin % 8 == 0 && k.We >= (g_tuning[HDU_TUNE_HALO_MIN_W] > 0 ? g_tuning[HDU_TUNE_HALO_MIN_W] : 24) &&      // (swept 32 / 24 / 14: r04_experiment_halo_wgrad_3d.txt)
         // operands through buffer resources with 32-bit byte offsets: over the whole tensor below 4 GiB, per input / output
         // plane above (round 5) -- a plane (+ one tile row of slack for the halo offsets) must stay inside 2^31 bytes
         ((long long)k.Hi * k.Wi + k.Wi + 2) * k.ldx * 2 < (1ll << 31) && ((long long)k.He * k.We + k.We + 2) * k.ldy * 2 < (1ll << 31);
}

// work grid of the halo-tile filter gradient: 32-channel chunks x filter-row tiles x splits of the spatial tiles
// (>= 2 tiles per workgroup).  Returns the tiles per split.
static int wgrad_halo_geometry(const ConvK& k, int BCO, int target, ConvK* kk, int min_tiles = 2) {
  const int tiles = k.N * k.Do * ((k.He + 3) / 4) * ((k.We + 31) / 32);
  const unsigned gx = (unsigned)((k.Cin + 31) / 32), gy = (unsigned)((k.Cout + BCO - 1) / BCO);      // (a ragged last chunk: zero-filled lanes)
  int want = target / (int)(gx * gy * (unsigned)k.KD);
  if (want < 1) want = 1;
  if (min_tiles < 1) min_tiles = 1;
  if (want > (tiles + min_tiles - 1) / min_tiles) want = (tiles + min_tiles - 1) / min_tiles;      // every workgroup ends with 9 x 32 x BCO float atomics
  if (want < 1) want = 1;
  const int per = (tiles + want - 1) / want;
  const unsigned gz = (unsigned)((tiles + per - 1) / per) * (unsigned)k.KD;      // (split, depth tap) pairs: wgrad_halo_body
  *kk = k;
  kk->wg_gx = (int)gx; kk->wg_gy = (int)gy; kk->wg_gz = (int)gz;
  return per;
}

template <int BCO>
static void launch_wgrad_halo(const ConvK& k, float* dw, hipStream_t s) {
  const int target = g_tuning[HDU_TUNE_HALO_TARGET_WGS] > 0 ? g_tuning[HDU_TUNE_HALO_TARGET_WGS] : 512;
  ConvK kk;
  const int per = wgrad_halo_geometry(k, BCO, target, &kk);
  HDU_LAUNCH((conv_wgrad_halo_kernel<BCO>), dim3(wgrad_grid(kk)), dim3(256), 0, s, kk, dw, per);
}

template <typename T>
static void dispatch_wgrad(const ConvK& k, float* dw, hipStream_t s) {
  const int best = choose_wgrad(k);
  if (sizeof(T) == 2 && wgrad_halo_ok(k)) {
    if (best == 64) launch_wgrad_halo<64>(k, dw, s);
    else if (best == 48) launch_wgrad_halo<48>(k, dw, s);
    else launch_wgrad_halo<32>(k, dw, s);
    return;
  }
  if (sizeof(T) == 2) {
    if (best == 64) launch_wgrad_tr<64>(k, dw, s);
    else if (best == 48) launch_wgrad_tr<48>(k, dw, s);
    else launch_wgrad_tr<32>(k, dw, s);
    return;
  }
  if (best == 64) launch_wgrad<T, 64>(k, dw, s);
  else if (best == 48) launch_wgrad<T, 48>(k, dw, s);
  else launch_wgrad<T, 32>(k, dw, s);
}

extern "C" int hdu_conv_wgrad(const hdu_conv_desc* d, float* dw, void* stream) {
  ConvK k;
  if (int e = fill_convk(d, &k, true)) return e;
  if (!dw || !d->y) return hdu_set_error(HDU_ERR_ARG, "conv_wgrad: null dw / dy");
  if ((uintptr_t)d->y % 16) return hdu_set_error(HDU_ERR_ARG, "conv_wgrad: dy must be 16-byte aligned");
  if (k.M == 0) return 0;
  if (hdu_stem_wgrad_launch(k, d->dtype, dw, (hipStream_t)stream)) return hdu_check_launch("conv_wgrad(stem)");
  if (d->dtype == HDU_BF16) dispatch_wgrad<bf16_t>(k, dw, (hipStream_t)stream);
  else dispatch_wgrad<float>(k, dw, (hipStream_t)stream);
  return hdu_check_launch("conv_wgrad");
}

// ---- batched filter gradients (see conv_wgrad_*_batched_kernel).  Variant id = kernel family of an entry:
// 0..5 DMA form <BCO, PW> = (64|48|32) x (false|true); 6 / 7 pointwise <64, true> with 3 / 2 filter-row tiles per workgroup;
// 8..10 halo-tile form <64|48|32>.
extern "C" size_t hdu_wgrad_plan_entry_bytes(void) { return sizeof(WgradEntry); }

extern "C" int hdu_wgrad_plan_fill(const hdu_conv_desc* d, float* dw, int target_wgs, int min_steps, void* entry, int* variant,
                                   uint32_t* nblocks) {
  if (!d || !dw || !entry || !variant || !nblocks) return hdu_set_error(HDU_ERR_ARG, "wgrad_plan_fill: null pointer");
  ConvK k;
  if (int e = fill_convk(d, &k, true)) return e;
  if (d->dtype != HDU_BF16 || !wgrad_dma_ok(k) || k.M == 0 || !d->y || (uintptr_t)d->y % 16)
    return hdu_set_error(HDU_ERR_ARG, "wgrad_plan_fill: only bf16 layers with materialised inputs (or pointwise layers with a BN prologue) and a 16-byte aligned dy can be batched");
  WgradEntry* e = (WgradEntry*)entry;
  const int best = choose_wgrad(k);
  const int bi = best == 64 ? 0 : (best == 48 ? 1 : 2);
  if (wgrad_halo_ok(k)) {
    const int target = target_wgs > 0 ? target_wgs : (g_tuning[HDU_TUNE_HALO_TARGET_WGS] > 0 ? g_tuning[HDU_TUNE_HALO_TARGET_WGS] : 512);
    e->per = wgrad_halo_geometry(k, best, target, &e->k, min_steps > 0 ? min_steps : 2);      // (batched: min_steps = spatial tiles per workgroup)
    *variant = 8 + bi;
  } else {
    const int target = target_wgs > 0 ? target_wgs : (g_tuning[HDU_TUNE_WGRAD_TARGET_WGS] > 0 ? g_tuning[HDU_TUNE_WGRAD_TARGET_WGS] : 768);
    const int nct = wgrad_nct(k, best);
    e->per = wgrad_dma_geometry(k, best, target, &e->k, min_steps > 0 ? min_steps : 8, nct);   // batched: other layers fill the chip, fewer atomics win (swept)
    *variant = nct == 3 ? 6 : (nct == 2 ? 7 : bi * 2 + (wgrad_pointwise(k) ? 1 : 0));
  }
  e->dw = dw;
  *nblocks = wgrad_grid(e->k);
  return 0;
}

extern "C" int hdu_wgrad_plan_shape(const hdu_conv_desc* d, int* variant, uint32_t* tiles, uint32_t* steps) {
  if (!d || !variant || !tiles || !steps) return hdu_set_error(HDU_ERR_ARG, "wgrad_plan_shape: null pointer");
  ConvK k;
  if (int e = fill_convk(d, &k, true)) return e;
  if (d->dtype != HDU_BF16 || !wgrad_dma_ok(k) || k.M == 0)
    return hdu_set_error(HDU_ERR_ARG, "wgrad_plan_shape: not a layer hdu_wgrad_plan_fill accepts");
  const int best = choose_wgrad(k);
  const int bi = best == 64 ? 0 : (best == 48 ? 1 : 2);
  if (wgrad_halo_ok(k)) {
    *variant = 8 + bi;
    *tiles = (uint32_t)((k.Cin + 31) / 32) * (uint32_t)((k.Cout + best - 1) / best) * (uint32_t)k.KD;
    *steps = (uint32_t)(k.N * k.Do * ((k.He + 3) / 4) * ((k.We + 31) / 32));
  } else {
    const int nct = wgrad_nct(k, best);
    *variant = nct == 3 ? 6 : (nct == 2 ? 7 : bi * 2 + (wgrad_pointwise(k) ? 1 : 0));
    *tiles = (uint32_t)((k.Ktot + 127) / 128) * (uint32_t)((k.Cout + best * nct - 1) / (best * nct));
    *steps = (uint32_t)((k.M + 63) / 64);
  }
  return 0;
}

extern "C" int hdu_wgrad_plan_run(int variant, const void* dev_entries, const uint32_t* dev_begins, int n,
                                  uint32_t total_blocks, void* stream) {
  if (!dev_entries || !dev_begins || n <= 0 || total_blocks == 0) return hdu_set_error(HDU_ERR_ARG, "wgrad_plan_run: bad args");
  const WgradEntry* tab = (const WgradEntry*)dev_entries;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g(total_blocks), b(256);
  switch (variant) {
    case 0: HDU_LAUNCH((conv_wgrad_dma_batched_kernel<64, false>), g, b, 0, s, tab, dev_begins, n); break;
    case 1: HDU_LAUNCH((conv_wgrad_dma_batched_kernel<64, true>), g, b, 0, s, tab, dev_begins, n); break;
    case 2: HDU_LAUNCH((conv_wgrad_dma_batched_kernel<48, false>), g, b, 0, s, tab, dev_begins, n); break;
    case 3: HDU_LAUNCH((conv_wgrad_dma_batched_kernel<48, true>), g, b, 0, s, tab, dev_begins, n); break;
    case 4: HDU_LAUNCH((conv_wgrad_dma_batched_kernel<32, false>), g, b, 0, s, tab, dev_begins, n); break;
    case 5: HDU_LAUNCH((conv_wgrad_dma_batched_kernel<32, true>), g, b, 0, s, tab, dev_begins, n); break;
    case 6: HDU_LAUNCH((conv_wgrad_dma_batched_kernel<64, true, 3>), g, b, 0, s, tab, dev_begins, n); break;
    case 7: HDU_LAUNCH((conv_wgrad_dma_batched_kernel<64, true, 2>), g, b, 0, s, tab, dev_begins, n); break;
    case 8: HDU_LAUNCH((conv_wgrad_halo_batched_kernel<64>), g, b, 0, s, tab, dev_begins, n); break;
    case 9: HDU_LAUNCH((conv_wgrad_halo_batched_kernel<48>), g, b, 0, s, tab, dev_begins, n); break;
    case 10: HDU_LAUNCH((conv_wgrad_halo_batched_kernel<32>), g, b, 0, s, tab, dev_begins, n); break;
    default: return hdu_set_error(HDU_ERR_ARG, "wgrad_plan_run: unknown variant");
  }
  return hdu_check_launch("wgrad_plan_run");
}

extern "C" int hdu_conv_dgrad_strided(const hdu_conv_desc* d, void* stream) {
  ConvK k;
  if (int e = fill_convk(d, &k, false, true)) return e;
  if (d->ud | d->uh | d->uw) return hdu_set_error(HDU_ERR_ARG, "conv_dgrad_strided: upsampled input not supported");
  if (!d->x || !d->y) return hdu_set_error(HDU_ERR_ARG, "conv_dgrad_strided: null dx / dy");
  if (d->epi_a) return hdu_set_error(HDU_ERR_ARG, "conv_dgrad_strided: no output affine");
  const long long total = (long long)d->N * d->Di * d->Hi * d->Wi * (d->Cin / (d->dtype == HDU_BF16 ? 8 : 4));
  if (total == 0) return 0;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (d->dtype == HDU_BF16)
    HDU_LAUNCH((conv_dgrad_strided_kernel<bf16_t>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k);
  else
    HDU_LAUNCH((conv_dgrad_strided_kernel<float>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k);
  return hdu_check_launch("conv_dgrad_strided");
}

static int parity_table(int KD, int KH, int KW, int sd, int sh, int sw, int pd, int ph, int pw, int Cin, int Cout,
                        ParityTable* tab) {
  const int K[3] = {KD, KH, KW}, S[3] = {sd, sh, sw}, P[3] = {pd, ph, pw};
  for (int a = 0; a < 3; ++a)
    if (S[a] != 1 && S[a] != 2) return -1;
  tab->n = sd * sh * sw;
  long long off = 0;
  for (int c = 0; c < tab->n; ++c) {
    const int r[3] = {c / (sh * sw), (c / sw) % sh, c % sw};
    ParityGeom& g = tab->c[c];
    for (int a = 0; a < 3; ++a) {
      g.step[a] = S[a];
      int kmax = K[a] - 1;
      if (S[a] == 2 && ((kmax - r[a] - P[a]) & 1)) --kmax;         // k = (r + p) mod 2
      g.kmax[a] = kmax;
      g.nt[a] = kmax < 0 ? 0 : kmax / S[a] + 1;
      if (g.nt[a] <= 0) return -1;
    }
    g.dst_off = off;
    off += (long long)Cin * g.nt[0] * g.nt[1] * g.nt[2] * Cout;
  }
  return 0;
}

extern "C" int hdu_stride2_dgrad_filters(int dtype, const float* w_master, int Cout, int KD, int KH, int KW, int Cin, int sd,
                                         int sh, int sw, int pd, int ph, int pw, void* w_out, void* stream) {
  ParityTable tab;
  if (!w_master || !w_out || Cout <= 0 || Cin <= 0 || parity_table(KD, KH, KW, sd, sh, sw, pd, ph, pw, Cin, Cout, &tab))
    return hdu_set_error(HDU_ERR_ARG, "stride2_dgrad_filters: bad args (strides must be 1 or 2)");
  const dim3 grid(64, (unsigned)tab.n);
  if (dtype == HDU_BF16)
    HDU_LAUNCH((stride2_filter_kernel<bf16_t>), grid, dim3(256), 0, (hipStream_t)stream, w_master, Cout, KD, KH, KW, Cin, tab, (bf16_t*)w_out);
  else if (dtype == HDU_F32)
    HDU_LAUNCH((stride2_filter_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, w_master, Cout, KD, KH, KW, Cin, tab, (float*)w_out);
  else
    return hdu_set_error(HDU_ERR_ARG, "stride2_dgrad_filters: bad dtype");
  return hdu_check_launch("stride2_dgrad_filters");
}

extern "C" int hdu_parity_interleave(int dtype, const void* cls, int N, int Di, int Hi, int Wi, int C, int sd, int sh, int sw,
                                     void* dx, int64_t lddx, int accumulate, void* stream) {
  const int ch = dtype == HDU_BF16 ? 8 : 4;
  if (!cls || !dx || N <= 0 || C <= 0 || C % ch || lddx % ch || Di % sd || Hi % sh || Wi % sw || (sd != 1 && sd != 2) ||
      (sh != 1 && sh != 2) || (sw != 1 && sw != 2))
    return hdu_set_error(HDU_ERR_ARG, "parity_interleave: bad args (dims must be multiples of the strides)");
  const long long total = (long long)N * Di * Hi * Wi * (C / ch);
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (dtype == HDU_BF16)
    HDU_LAUNCH((parity_interleave_kernel<bf16_t>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)cls,
               N, Di, Hi, Wi, C, sd, sh, sw, (bf16_t*)dx, (long long)lddx, accumulate);
  else if (dtype == HDU_F32)
    HDU_LAUNCH((parity_interleave_kernel<float>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)cls, N,
               Di, Hi, Wi, C, sd, sh, sw, (float*)dx, (long long)lddx, accumulate);
  else
    return hdu_set_error(HDU_ERR_ARG, "parity_interleave: bad dtype");
  return hdu_check_launch("parity_interleave");
}

extern "C" int hdu_weight_prep(int dtype, const float* w_master, int Cout, int T, int Cin, void* w_f, void* w_d,
                               void* stream) {
  if (!w_master || Cout <= 0 || T <= 0 || Cin <= 0) return hdu_set_error(HDU_ERR_ARG, "weight_prep: bad args");
  const long long total = (long long)Cout * T * Cin;
  long long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (dtype == HDU_BF16)
    HDU_LAUNCH((weight_prep_kernel<bf16_t>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w_master,
               Cout, T, Cin, (bf16_t*)w_f, (bf16_t*)w_d);
  else if (dtype == HDU_F32)
    HDU_LAUNCH((weight_prep_kernel<float>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w_master,
               Cout, T, Cin, (float*)w_f, (float*)w_d);
  else
    return hdu_set_error(HDU_ERR_ARG, "weight_prep: bad dtype");
  return hdu_check_launch("weight_prep");
}

#include <cstdio>
extern "C" int hdu_conv_kernel_name(const hdu_conv_desc* d, int op, char* buf, size_t buflen) {
  ConvK k;
  if (int e = fill_convk(d, &k, op == 1)) return e;
  if (!buf || buflen < 8) return hdu_set_error(HDU_ERR_ARG, "conv_kernel_name: bad buffer");
  // spelled exactly as rocprofv3 prints the instantiation (so bench.py's live numbers and profiles/ line up)
  const char* t = d->dtype == HDU_BF16 ? "unsigned short" : "float";
  if (op == 1) {
    const bool dma = wgrad_dma_ok(k);
    const bool pw = k.KD * k.KH * k.KW == 1 && k.sd == 1 && k.sh == 1 && k.sw == 1 && (k.pd | k.ph | k.pw) == 0 &&
                    (k.ud | k.uh | k.uw) == 0;
    if (hdu_stem_wgrad_taken(k, d->dtype)) snprintf(buf, buflen, "conv_stem_wgrad_kernel");
    else if (d->dtype == HDU_BF16 && wgrad_halo_ok(k)) snprintf(buf, buflen, "conv_wgrad_halo_kernel<%d>", choose_wgrad(k));
    else if (d->dtype == HDU_BF16 && dma) snprintf(buf, buflen, "conv_wgrad_dma_kernel<%d, %s>", choose_wgrad(k), pw ? "true" : "false");
    else if (d->dtype == HDU_BF16) snprintf(buf, buflen, "conv_wgrad_tr_kernel<%d>", choose_wgrad(k));
    else snprintf(buf, buflen, "conv_wgrad_kernel<float, %d>", choose_wgrad(k));
  } else if (pw_bstat_ok(k, d->dtype)) {
    if (pw_bstat_form(k) == 2) snprintf(buf, buflen, "conv_pw_bstat_kernel<%d, 64, %s, 2>", k.Ktot / 64, k.bnb_u ? "true" : "false");
    else snprintf(buf, buflen, "conv_pw_bstat_kernel<%d, 128, %s, 3>", k.Ktot / 64, k.bnb_u ? "true" : "false");
  } else if (hdu_halo_wide_taken(k, d->dtype)) {
    snprintf(buf, buflen, "%s", hdu_halo_wide_name(k, d->dtype));
  } else if (fprop_halo_ok(k, d->dtype)) {
    snprintf(buf, buflen, "conv_halo_fprop_kernel<%d>", choose_halo_bn(k));
  } else {
    int bm, bn;
    choose_igemm(k, &bm, &bn);
    if (bm == 128 && igemm_pers_ok(k, bn)) {
      snprintf(buf, buflen, "conv_igemm_pers_kernel<%s, %d, %d>", t, bn, k.pro_a ? pers_table_cap(bn, k.Cin) : 0);
      return 0;
    }
    const int wm = (bn >= 128) ? 2 : ((bm == 64 && (bn == 64 || bn == 32)) ? 2 : 4);
    const bool prodma = igemm_pro_dma_ok(k);
    const bool dma = prodma || (k.pro_a == nullptr && k.skip == nullptr && k.vec_out);
    const long long nblk = ((k.M_layer + bm - 1) / bm) * ((k.Cout + bn - 1) / bn);
    const int mode = g_tuning[HDU_TUNE_DMA_STAGES];
    const int stage = (bm + ((bn + 31) / 32) * 32) * 128;
    const int nsd = stage * 6 <= 160 * 1024 ? 6 : 4;
    const bool ring = dma && igemm_ring_ok(nblk, k.Ktot, stage, nsd);
    int nsr = (nsd == 6 && ring_wgs_per_cu(bm, d->dtype == HDU_BF16) == 2) ? 3 : nsd;     // (launch_igemm)
    const int proc = prodma ? (k.Cin <= HDU_PRO_CSMALL ? HDU_PRO_CSMALL : HDU_PRO_CMAX) : 0;
    if (prodma && nsr * stage + 8 * proc > 160 * 1024) nsr = nsr == 6 ? 4 : 3;
    const char* fast = igemm_fast_ok(k) ? "true" : "false";
    const char* bnb = k.bnb_u != nullptr ? "true" : "false";
    if (ring) snprintf(buf, buflen, "conv_igemm_ring_kernel<%s, %d, %d, %d, %d, %d, %s, %s, %d>", t, bm, bn, wm, 4 / wm, nsr, fast, bnb, proc);
    else if (dma) snprintf(buf, buflen, "conv_igemm_dma_kernel<%s, %d, %d, %d, %d, %s, %s, %d>", t, bm, bn, wm, 4 / wm, fast, bnb, proc);
    else snprintf(buf, buflen, "conv_igemm_kernel<%s, %d, %d, %d, %d>", t, bm, bn, wm, 4 / wm);
  }
  return 0;
}

extern "C" int hdu_weight_prep_batched(int dtype, const hdu_prep_entry* table, int n, int64_t total_tiles,
                                       const float* master_base, void* wc_base, void* stream) {
  if (!table || n <= 0 || total_tiles <= 0 || !master_base || !wc_base)
    return hdu_set_error(HDU_ERR_ARG, "weight_prep_batched: bad args");
  if (dtype == HDU_BF16)
    HDU_LAUNCH((weight_prep_batched_kernel<bf16_t>), dim3((unsigned)((total_tiles + HDU_PREP_TPW - 1) / HDU_PREP_TPW)), dim3(256), 0,
               (hipStream_t)stream, table, n, master_base, (bf16_t*)wc_base, (long long)total_tiles);
  else if (dtype == HDU_F32)
    HDU_LAUNCH((weight_prep_batched_kernel<float>), dim3((unsigned)((total_tiles + HDU_PREP_TPW - 1) / HDU_PREP_TPW)), dim3(256), 0,
               (hipStream_t)stream, table, n, master_base, (float*)wc_base, (long long)total_tiles);
  else
    return hdu_set_error(HDU_ERR_ARG, "weight_prep_batched: bad dtype");
  return hdu_check_launch("weight_prep_batched");
}
