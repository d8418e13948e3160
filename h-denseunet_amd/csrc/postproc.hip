// postproc.hip -- device-resident post-processing of the LiTS inference (test.py:52-112; host specification:
// h-denseunet_amd/funcs.py liver_window_from_mask / segment_liver_tumor).
//
// Every mask and label array is a volume in the host's raster order: [X][Y][Z] C-order, x = deps, z = cols, index
// i = (x * Y + y) * Z + z.  Only the threshold pass reads the sweep's score layout [z][deps][rows][num].
//
// Connected components are a lock-free union-find over a parent array with parent[i] <= i at all times: a union always
// links the LARGER root under the smaller one (one atomicMin on the larger root's word), and path halving only ever
// lowers a word to an ancestor.  Hence a root is the minimum raster index of its component whatever the schedule, no
// cycle can form and every find loop ends.  The launch sequence is fixed (no "until nothing changes" host loop):
//   1. runs: one thread per (x, y) column links every voxel of a z-run to the run's first voxel;
//   2. union: every voxel unites with its backward neighbours (those with a smaller raster index), except where the pair
//      one plane down (z - 1) is a neighbour pair of the same offset with both voxels set -- that pair's own union (or its
//      own skip, down to a pair that is united) together with the z-run links of step 1 already joins them;
//   3. flatten: parent[i] <- find(i), which is the component's minimum index.
// Reads of parent words in the union pass are relaxed agent-scope loads, which may return an older (larger or equal) value
// of a word another workgroup has lowered: such a value is still an ancestor, and every decision to stop is taken on the
// value an atomicMin returned, so a stale read costs one more iteration and never a wrong link.
#include "hdu_host.h"

#define PP_NONE 0xFFFFFFFFu

// ------------------------------------------------------------------ thresholds
// one workgroup = one x, a 64 (y) x 64 (z) tile: read with y fastest (the score layout), written with z fastest (raster)
__global__ __launch_bounds__(256) void pp_threshold_kernel(const float* __restrict__ score, const float* __restrict__ count,
                                                           int Y, int Z, int deps, int rows, int num, int lc, int tc,
                                                           double thres_liver, double thres_tumor,
                                                           uint8_t* __restrict__ liver, uint8_t* __restrict__ tumor) {
  __shared__ uint8_t tile[64][65];
  const int x = blockIdx.x, y0 = blockIdx.y * 64, z0 = blockIdx.z * 64;
  const int tid = threadIdx.x;
  for (int k = 0; k < 16; ++k) {
    const int e = k * 256 + tid, zl = e >> 6, yl = e & 63;
    const int y = y0 + yl, z = z0 + zl;
    if (y >= Y || z >= Z) continue;
    float sl = 0.f, st = 0.f;
    if (x < deps && y < rows) {
      const size_t off = (((size_t)z * deps + x) * rows + y) * num;
      const float den = count[z] + 1e-4f;    // score / (score_num + np.float32(1e-4)), float32, IEEE division
      sl = score[off + lc] / den;
      st = score[off + tc] / den;
    }
    const int t = (double)st >= thres_tumor;
    const int l = (double)sl >= thres_liver;
    tile[yl][zl] = (uint8_t)(l | (t << 1));
  }
  __syncthreads();
  for (int k = 0; k < 16; ++k) {
    const int e = k * 256 + tid, yl = e >> 6, zl = e & 63;
    const int y = y0 + yl, z = z0 + zl;
    if (y >= Y || z >= Z) continue;
    const unsigned v = tile[yl][zl];
    const size_t i = ((size_t)x * Y + y) * Z + z;
    tumor[i] = (uint8_t)(v >> 1);
    liver[i] = (uint8_t)((v | (v >> 1)) & 1u);
  }
}

// ------------------------------------------------------------------ binary dilation, 6-connected cross, border 0
__global__ __launch_bounds__(256) void pp_dilate_kernel(const uint8_t* __restrict__ in, int X, int Y, int Z, long long N,
                                                        uint8_t* __restrict__ out) {
  const long long YZ = (long long)Y * Z;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    const int z = (int)(i % Z);
    const long long t = i / Z;
    const int y = (int)(t % Y), x = (int)(t / Y);
    bool v = in[i] != 0;
    v = v || (z > 0 && in[i - 1]) || (z < Z - 1 && in[i + 1]);
    v = v || (y > 0 && in[i - Z]) || (y < Y - 1 && in[i + Z]);
    v = v || (x > 0 && in[i - YZ]) || (x < X - 1 && in[i + YZ]);
    out[i] = (uint8_t)v;
  }
}

// ------------------------------------------------------------------ connected components
__device__ __forceinline__ bool pp_fg(const uint8_t* mask, long long i, int background) {
  return (mask[i] != 0) != (background != 0);
}

// step 1: parent[i] = first voxel of i's z-run (PP_NONE off the labelled set)
__global__ __launch_bounds__(256) void pp_label_runs_kernel(const uint8_t* __restrict__ mask, long long cols, int Z, int background,
                                                            unsigned* __restrict__ parent) {
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cols; c += (long long)gridDim.x * blockDim.x) {
    const long long base = c * Z;
    unsigned start = PP_NONE;
    for (int z = 0; z < Z; ++z) {
      const bool v = pp_fg(mask, base + z, background);
      if (!v) start = PP_NONE;
      else if (start == PP_NONE) start = (unsigned)(base + z);
      parent[base + z] = v ? start : PP_NONE;
    }
  }
}

__device__ __forceinline__ unsigned pp_find(unsigned* parent, unsigned x) {
  for (;;) {
    const unsigned px = hdu_load_relaxed_u32(parent + x);
    if (px == x) return x;
    const unsigned ppx = hdu_load_relaxed_u32(parent + px);
    if (ppx != px) hdu_atomic_min_u32(parent + x, ppx);   // path halving: lowers x's word to an ancestor
    x = ppx;
  }
}

__device__ __forceinline__ void pp_unite(unsigned* parent, unsigned a, unsigned b) {
  for (;;) {
    a = pp_find(parent, a);
    b = pp_find(parent, b);
    if (a == b) return;
    if (a < b) { const unsigned t = a; a = b; b = t; }
    const unsigned old = hdu_atomic_min_u32(parent + a, b);   // the larger root goes under the smaller one
    if (old == a) return;                                     // a was still a root: linked
    a = old;                                                  // a had been linked meanwhile: join its new parent instead
  }
}

// step 2.  Backward neighbours (dx, dy, dz) with a smaller raster index, the z-run link (0, 0, -1) excluded: 6-connectivity
// (-1,0,0), (0,-1,0); 26-connectivity the 9 offsets with dx = -1 and the 3 with dx = 0, dy = -1.
__global__ __launch_bounds__(256) void pp_label_union_kernel(const uint8_t* __restrict__ mask, int X, int Y, int Z, long long N,
                                                             int conn26, int background, unsigned* __restrict__ parent) {
  const long long YZ = (long long)Y * Z;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    if (!pp_fg(mask, i, background)) continue;
    const int z = (int)(i % Z);
    const long long t = i / Z;
    const int y = (int)(t % Y), x = (int)(t / Y);
    const bool below = z > 0 && pp_fg(mask, i - 1, background);
    const int noff = conn26 ? 12 : 2;
    for (int k = 0; k < noff; ++k) {
      int dx, dy, dz;
      if (conn26) {
        if (k < 9) { dx = -1; dy = k / 3 - 1; dz = k % 3 - 1; }
        else { dx = 0; dy = -1; dz = k - 10; }
      } else {
        dx = k == 0 ? -1 : 0; dy = k == 0 ? 0 : -1; dz = 0;
      }
      if (x + dx < 0 || y + dy < 0 || y + dy >= Y || z + dz < 0 || z + dz >= Z) continue;
      const long long n = i + dx * YZ + dy * (long long)Z + dz;
      if (!pp_fg(mask, n, background)) continue;
      if (below && z + dz > 0 && pp_fg(mask, n - 1, background)) continue;   // implied by the pair (i - 1, n - 1)
      pp_unite(parent, (unsigned)i, (unsigned)n);
    }
  }
}

// step 3.  No union runs any more: every word holds an ancestor, words of non-roots are below their own index, and the
// only stores are of final roots, so the walk ends at the root whichever versions it reads.
__global__ __launch_bounds__(256) void pp_label_flatten_kernel(long long N, unsigned* __restrict__ parent) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    unsigned p = parent[i];
    if (p == PP_NONE || p == (unsigned)i) continue;
    for (;;) {
      const unsigned q = hdu_load_relaxed_u32(parent + p);
      if (q == p) break;
      p = q;
    }
    parent[i] = p;
  }
}

// ------------------------------------------------------------------ largest component
// area[root] += voxels; a thread walks PP_AREA_RUN consecutive voxels and adds once per run of one root
#define PP_AREA_RUN 16
__global__ __launch_bounds__(256) void pp_area_kernel(const unsigned* __restrict__ root, long long N, unsigned* __restrict__ area) {
  const long long chunks = (N + PP_AREA_RUN - 1) / PP_AREA_RUN;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (long long)gridDim.x * blockDim.x) {
    const long long i0 = c * PP_AREA_RUN, i1 = i0 + PP_AREA_RUN < N ? i0 + PP_AREA_RUN : N;
    unsigned cur = PP_NONE, cnt = 0;
    for (long long i = i0; i < i1; ++i) {
      const unsigned r = root[i];
      if (r != cur) {
        if (cur != PP_NONE) atomicAdd(area + cur, cnt);
        cur = r;
        cnt = 0;
      }
      ++cnt;
    }
    if (cur != PP_NONE) atomicAdd(area + cur, cnt);
  }
}

// best = max over roots r of (area[r] << 32) | (0xFFFFFFFF - r): the largest area, on a tie the component whose first voxel
// comes first in raster order (skimage labels in raster order + `box.index(max(box)) + 1`, test.py:84-92); ncomp += roots
__global__ __launch_bounds__(256) void pp_winner_kernel(const unsigned* __restrict__ root, const unsigned* __restrict__ area,
                                                        long long N, unsigned long long* best, unsigned* ncomp) {
  __shared__ unsigned long long smax[256];
  __shared__ unsigned scnt[256];
  unsigned long long m = 0;
  unsigned cnt = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    if (root[i] != (unsigned)i) continue;
    const unsigned long long key = ((unsigned long long)area[i] << 32) | (unsigned long long)(PP_NONE - (unsigned)i);
    m = key > m ? key : m;
    ++cnt;
  }
  smax[threadIdx.x] = m;
  scnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      smax[threadIdx.x] = smax[threadIdx.x + st] > smax[threadIdx.x] ? smax[threadIdx.x + st] : smax[threadIdx.x];
      scnt[threadIdx.x] += scnt[threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && scnt[0]) {
    hdu_atomic_max_u64(best, smax[0]);
    atomicAdd(ncomp, scnt[0]);
  }
}

__global__ __launch_bounds__(256) void pp_keep_kernel(const unsigned* __restrict__ root, long long N, const unsigned long long* best,
                                                      uint8_t* __restrict__ out) {
  const unsigned long long b = *best;
  const unsigned win = PP_NONE - (unsigned)b;      // b == 0 (no component): win = PP_NONE, which no voxel keeps
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    const unsigned r = root[i];
    out[i] = (uint8_t)(b != 0 && r == win);
  }
}

// ------------------------------------------------------------------ hole filling (ndimage.binary_fill_holes)
// flag[r] = 1 for every background root r with a voxel on a face of the volume
__global__ __launch_bounds__(256) void pp_border_kernel(const unsigned* __restrict__ root, int X, int Y, int Z, uint8_t* __restrict__ flag) {
  const long long fx = (long long)Y * Z, fy = (long long)X * Z, fz = (long long)X * Y;
  const long long total = 2 * (fx + fy + fz);
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    long long u = t;
    int x, y, z;
    if (u < 2 * fx) { x = u < fx ? 0 : X - 1; u %= fx; y = (int)(u / Z); z = (int)(u % Z); }
    else if ((u -= 2 * fx) < 2 * fy) { y = u < fy ? 0 : Y - 1; u %= fy; x = (int)(u / Z); z = (int)(u % Z); }
    else { u -= 2 * fy; z = u < fz ? 0 : Z - 1; u %= fz; x = (int)(u / Y); y = (int)(u % Y); }
    const unsigned r = root[((long long)x * Y + y) * Z + z];
    if (r != PP_NONE) flag[r] = 1;
  }
}

__global__ __launch_bounds__(256) void pp_fill_compose_kernel(const uint8_t* __restrict__ mask, const unsigned* __restrict__ root,
                                                              const uint8_t* __restrict__ flag, long long N, uint8_t* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    const unsigned r = root[i];
    out[i] = (uint8_t)(mask[i] != 0 || (r != PP_NONE && !flag[r]));
  }
}

// ------------------------------------------------------------------ bounding box of the set voxels
__global__ __launch_bounds__(256) void pp_bbox_kernel(const uint8_t* __restrict__ mask, int Y, int Z, long long N, unsigned* box) {
  __shared__ unsigned s[6][256];
  unsigned lo[3] = {PP_NONE, PP_NONE, PP_NONE}, hi[3] = {0, 0, 0};
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    if (!mask[i]) continue;
    const long long t = i / Z;
    const unsigned c[3] = {(unsigned)(t / Y), (unsigned)(t % Y), (unsigned)(i % Z)};
    for (int a = 0; a < 3; ++a) { lo[a] = c[a] < lo[a] ? c[a] : lo[a]; hi[a] = c[a] > hi[a] ? c[a] : hi[a]; }
  }
  for (int a = 0; a < 3; ++a) { s[a][threadIdx.x] = lo[a]; s[3 + a][threadIdx.x] = hi[a]; }
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      for (int a = 0; a < 3; ++a) {
        const unsigned l2 = s[a][threadIdx.x + st], h2 = s[3 + a][threadIdx.x + st];
        s[a][threadIdx.x] = l2 < s[a][threadIdx.x] ? l2 : s[a][threadIdx.x];
        s[3 + a][threadIdx.x] = h2 > s[3 + a][threadIdx.x] ? h2 : s[3 + a][threadIdx.x];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && s[0][0] != PP_NONE) {
    for (int a = 0; a < 3; ++a) { hdu_atomic_min_u32(box + a, s[a][0]); hdu_atomic_max_u32(box + 3 + a, s[3 + a][0]); }
  }
}

// ------------------------------------------------------------------ element-wise composition
__global__ __launch_bounds__(256) void pp_merge_kernel(int op, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, long long N,
                                                       uint8_t* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    const bool av = a[i] != 0, bv = b[i] != 0;
    out[i] = op == HDU_PP_AND ? (uint8_t)(av && bv) : (uint8_t)(bv ? 2 : (av ? 1 : 0));
  }
}

// ------------------------------------------------------------------ label planes of the 2-D slice sweep -> raster order
// labels uint8 [Z][H][W] (the argmax planes of hdu_slice_argmax_store) -> out uint8 [X][Y][Z], zero outside the H x W window.
// For one x this is a byte transpose [Z][W] -> [W][Z].  One workgroup = one x, a 64 (z) x 64 (y) tile held in LDS as
// tile[y][z / 4]: one 32-bit word = the bytes of four consecutive z, the unit the raster order stores.
//   read phase:  a wave holds one z-quad and 64 consecutive y: four byte loads per lane, each a 64-byte run along y, packed into
//                ONE ds_write_b32 at word 17 * y + zq.  The row pitch of 17 words is odd, so the 32 lanes of a half-wave
//                (consecutive y) fall on 32 different banks.
//   write phase: 16 lanes = the 16 z-quads of one y: one 64-byte run along z per y.  The four y of a wave are 16 rows apart:
//                a half-wave reads the words 17 * y + 0..15 and 17 * (y + 16) + 0..15 = 17 * y + 16 + 0..15 (mod 32), again 32
//                different banks.  The word is stored whole where it is aligned and inside Z, byte by byte otherwise.
#define PP_RASTER_PITCH 17
__global__ __launch_bounds__(256) void slice_labels_to_raster_kernel(const uint8_t* __restrict__ labels, int Y, int Z, int H, int W,
                                                                     uint8_t* __restrict__ out) {
  __shared__ unsigned tile[64 * PP_RASTER_PITCH];
  const int x = blockIdx.x, y0 = blockIdx.y * 64, z0 = blockIdx.z * 64;
  const int tid = threadIdx.x;
  for (int k = 0; k < 4; ++k) {
    const int e = k * 256 + tid, zq = e >> 6, yl = e & 63;
    const int y = y0 + yl;
    unsigned word = 0;
    if (x < H && y < W) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int z = z0 + 4 * zq + j;
        if (z < Z) word |= (unsigned)labels[((size_t)z * H + x) * W + y] << (8 * j);
      }
    }
    tile[yl * PP_RASTER_PITCH + zq] = word;
  }
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    const int zq = tid & 15, yl = k * 4 + (tid >> 6) + 16 * ((tid >> 4) & 3);
    const int y = y0 + yl, z = z0 + 4 * zq;
    if (y >= Y || z >= Z) continue;
    const unsigned word = tile[yl * PP_RASTER_PITCH + zq];
    uint8_t* __restrict__ o = out + ((size_t)x * Y + y) * Z + z;
    if (z + 3 < Z && ((uintptr_t)o & 3u) == 0) {
      *(unsigned*)o = word;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (z + j < Z) o[j] = (uint8_t)(word >> (8 * j));
    }
  }
}

// ------------------------------------------------------------------ C-ABI (include/hdu.h)
#define PP_LAUNCH(kern, n, ...) HDU_LAUNCH(kern, dim3(hdu_grid_1d((n), 256, 8192)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__)

static int pp_check_dims(int X, int Y, int Z, const char* what, long long* N) {
  if (X <= 0 || Y <= 0 || Z <= 0) return hdu_set_error(HDU_ERR_ARG, what);
  const long long n = (long long)X * Y * Z;
  if (n >= (long long)PP_NONE) return hdu_set_error(HDU_ERR_ARG, "post-processing: volumes of 2^32 - 1 voxels or more are not supported");
  *N = n;
  return 0;
}

extern "C" int hdu_pp_threshold(const float* score, const float* count, int X, int Y, int Z, int deps, int rows, int num,
                                double thres_liver, double thres_tumor, uint8_t* liver, uint8_t* tumor, void* stream) {
  long long N;
  if (int e = pp_check_dims(X, Y, Z, "pp_threshold: bad volume dims", &N)) return e;
  if (!score || !count || !liver || !tumor || num < 1 || num > 3 || deps < 0 || rows < 0 || deps > X || rows > Y)
    return hdu_set_error(HDU_ERR_ARG, "pp_threshold: bad args");
  // funcs.predict_tumor_inwindow returns channels num - 2 and num - 1 (Python indices: -1 is the last channel)
  const int lc = num >= 2 ? num - 2 : num - 1, tc = num - 1;
  HDU_LAUNCH(pp_threshold_kernel, dim3(X, (Y + 63) / 64, (Z + 63) / 64), dim3(256), 0, (hipStream_t)stream, score, count, Y, Z, deps,
             rows, num, lc, tc, thres_liver, thres_tumor, liver, tumor);
  return hdu_check_launch("pp_threshold");
}

extern "C" int hdu_pp_dilate(const uint8_t* in, int X, int Y, int Z, uint8_t* out, void* stream) {
  long long N;
  if (int e = pp_check_dims(X, Y, Z, "pp_dilate: bad volume dims", &N)) return e;
  if (!in || !out || in == out) return hdu_set_error(HDU_ERR_ARG, "pp_dilate: bad args (in-place not supported)");
  PP_LAUNCH(pp_dilate_kernel, N, in, X, Y, Z, N, out);
  return hdu_check_launch("pp_dilate");
}

static int pp_label(const uint8_t* mask, int X, int Y, int Z, long long N, int conn26, int background, unsigned* root, void* stream) {
  const long long cols = (long long)X * Y;
  PP_LAUNCH(pp_label_runs_kernel, cols, mask, cols, Z, background, root);
  if (int e = hdu_check_launch("pp_label (runs)")) return e;
  PP_LAUNCH(pp_label_union_kernel, N, mask, X, Y, Z, N, conn26, background, root);
  if (int e = hdu_check_launch("pp_label (union)")) return e;
  PP_LAUNCH(pp_label_flatten_kernel, N, N, root);
  return hdu_check_launch("pp_label (flatten)");
}

extern "C" int hdu_pp_label(const uint8_t* mask, int X, int Y, int Z, int connectivity, int background, uint32_t* root, void* stream) {
  long long N;
  if (int e = pp_check_dims(X, Y, Z, "pp_label: bad volume dims", &N)) return e;
  if (!mask || !root || (connectivity != 6 && connectivity != 26)) return hdu_set_error(HDU_ERR_ARG, "pp_label: bad args (connectivity 6 or 26)");
  return pp_label(mask, X, Y, Z, N, connectivity == 26, background, root, stream);
}

extern "C" int hdu_pp_largest(const uint32_t* root, int X, int Y, int Z, uint32_t* area, uint64_t* best, uint32_t* ncomp, uint8_t* out,
                              void* stream) {
  long long N;
  if (int e = pp_check_dims(X, Y, Z, "pp_largest: bad volume dims", &N)) return e;
  if (!root || !area || !best || !ncomp || !out) return hdu_set_error(HDU_ERR_ARG, "pp_largest: bad args");
  PP_LAUNCH(pp_area_kernel, (N + PP_AREA_RUN - 1) / PP_AREA_RUN, root, N, area);
  if (int e = hdu_check_launch("pp_largest (area)")) return e;
  PP_LAUNCH(pp_winner_kernel, N, root, area, N, (unsigned long long*)best, ncomp);
  if (int e = hdu_check_launch("pp_largest (winner)")) return e;
  PP_LAUNCH(pp_keep_kernel, N, root, N, (const unsigned long long*)best, out);
  return hdu_check_launch("pp_largest (keep)");
}

extern "C" int hdu_pp_fill_holes(const uint8_t* mask, int X, int Y, int Z, uint32_t* root, uint8_t* flag, uint8_t* out, void* stream) {
  long long N;
  if (int e = pp_check_dims(X, Y, Z, "pp_fill_holes: bad volume dims", &N)) return e;
  if (!mask || !root || !flag || !out) return hdu_set_error(HDU_ERR_ARG, "pp_fill_holes: bad args");
  if (int e = pp_label(mask, X, Y, Z, N, 0, 1, root, stream)) return e;
  const long long faces = 2 * ((long long)Y * Z + (long long)X * Z + (long long)X * Y);
  PP_LAUNCH(pp_border_kernel, faces, root, X, Y, Z, flag);
  if (int e = hdu_check_launch("pp_fill_holes (border)")) return e;
  PP_LAUNCH(pp_fill_compose_kernel, N, mask, root, flag, N, out);
  return hdu_check_launch("pp_fill_holes (compose)");
}

extern "C" int hdu_pp_bbox(const uint8_t* mask, int X, int Y, int Z, uint32_t* box, void* stream) {
  long long N;
  if (int e = pp_check_dims(X, Y, Z, "pp_bbox: bad volume dims", &N)) return e;
  if (!mask || !box) return hdu_set_error(HDU_ERR_ARG, "pp_bbox: bad args");
  PP_LAUNCH(pp_bbox_kernel, N, mask, Y, Z, N, box);
  return hdu_check_launch("pp_bbox");
}

extern "C" int hdu_pp_merge(int op, const uint8_t* a, const uint8_t* b, int64_t n, uint8_t* out, void* stream) {
  if (!a || !b || !out || n < 0 || (op != HDU_PP_AND && op != HDU_PP_LABEL)) return hdu_set_error(HDU_ERR_ARG, "pp_merge: bad args");
  if (n == 0) return 0;
  PP_LAUNCH(pp_merge_kernel, n, op, a, b, (long long)n, out);
  return hdu_check_launch("pp_merge");
}

extern "C" int hdu_slice_labels_to_raster(const uint8_t* labels, int X, int Y, int Z, int H, int W, uint8_t* out, void* stream) {
  long long N;
  if (int e = pp_check_dims(X, Y, Z, "slice_labels_to_raster: bad volume dims", &N)) return e;
  if (!labels || !out || labels == out) return hdu_set_error(HDU_ERR_ARG, "slice_labels_to_raster: bad args (in-place not supported)");
  if (H < 1 || W < 1 || H > X || W > Y) return hdu_set_error(HDU_ERR_ARG, "slice_labels_to_raster: bad args (1 <= H <= X, 1 <= W <= Y)");
  if ((Z + 63) / 64 > 65535 || (Y + 63) / 64 > 65535)
    return hdu_set_error(HDU_ERR_ARG, "slice_labels_to_raster: bad args (Y and Z below 64 * 65536)");
  HDU_LAUNCH(slice_labels_to_raster_kernel, dim3(X, (Y + 63) / 64, (Z + 63) / 64), dim3(256), 0, (hipStream_t)stream, labels, Y, Z,
             H, W, out);
  return hdu_check_launch("slice_labels_to_raster");
}
