// Connected-component post-processing of a predicted label map (tta/postprocessing.py): canonical multi-label component
// labelling under 6 / 18 / 26 connectivity, component sizes, and the keep-largest / minimum-size filter.  Everything is integer
// valued and canonical (a component is named by its smallest linear index), so the results do not depend on the scheduling.
// The same labelling, run on the complement of a uint8 mask, fills holes (fill_label_holes, the non-zero crop of preprocessing.py).
#include "conv_api.h"

#include <limits.h>

namespace {

constexpr int CC_MAXTAB = DGTTA_CC_MAX_TABLE;  // group table in LDS: 4 KB
constexpr int TD = 8, TH = 8, TW = WAVE;       // tile of the local pass: a wave owns a row, a workgroup 64 rows
constexpr int TV = TD * TH * TW;

// the backward neighbours (smaller linear index) as (dd, dh, dw): 3 faces, then 6 edges, then 4 corners
__constant__ const signed char CC_OFF[13][3] = {{0, 0, -1},  {0, -1, 0},  {-1, 0, 0},  {0, -1, -1}, {0, -1, 1},  {-1, 0, -1}, {-1, 0, 1},
                                                {-1, -1, 0}, {-1, 1, 0},  {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

// group ids outside [0, ntab) count as 0, so that a group id can index every per-group table
__device__ __forceinline__ void load_groups(int *sgroup, const int *__restrict__ group, int ntab) {
  for (int i = threadIdx.x; i < ntab; i += blockDim.x) {
    const int g = group[i];
    sgroup[i] = (unsigned)g < (unsigned)ntab ? g : 0;
  }
}
__device__ __forceinline__ int group_of(int64_t m, const int *sgroup, int ntab) { return (uint64_t)m < (uint64_t)ntab ? sgroup[m] : 0; }

// What the labelling kernels take a voxel's group from: a label map looked up in the group table staged in LDS (cc_label), or a
// uint8 mask whose ZERO voxels are the one group (holes_fill labels the complement).
struct MapGroups {
  const int64_t *map;
  const int *group;
  int ntab;
  static constexpr int LDS = CC_MAXTAB;
  __device__ __forceinline__ void load(int *sgroup) const { load_groups(sgroup, group, ntab); }
  __device__ __forceinline__ int at(int64_t i, const int *sgroup) const { return group_of(map[i], sgroup, ntab); }
};
struct MaskComplement {
  const uint8_t *mask;
  static constexpr int LDS = 1;
  __device__ __forceinline__ void load(int *) const {}
  __device__ __forceinline__ int at(int64_t i, const int *) const { return mask[i] == 0; }
};

// ============================================================================ union-find
// parent[x] <= x always, and only members of x's component are ever stored there; the larger root hangs under the smaller, so
// the root of a finished tree is the component's smallest index.
__device__ __forceinline__ int lds_find(const volatile int *p, int x) {
  int q;
  while ((q = p[x]) != x) x = q;
  return x;
}

__device__ __forceinline__ void lds_union(int *p, int a, int b) {
  for (;;) {
    a = lds_find(p, a), b = lds_find(p, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(&p[a], b);
    if (old == a) return;                      // a was a root and now hangs under b
    a = old;                                   // it was not: old and b remain to be united
  }
}

// The global forest is united by workgroups on all eight XCDs at once, whose loads may return a value that another workgroup
// has lowered since.  A stale value is an earlier content of the same word: still <= x and still of x's component, so find
// terminates and returns SOME member.  Whether that member was a root is decided by the value the atomicMin returns, never by a
// load; when it was not, the link that the atomicMin may have replaced (x -> old) is made up for by going on with (old, b).
__device__ __forceinline__ int glb_find(const int *p, int x) {
  int q;
  while ((q = __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = q;
  return x;
}

__device__ __forceinline__ void glb_union(int *p, int a, int b) {
  for (;;) {
    a = glb_find(p, a), b = glb_find(p, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(&p[a], b);
    if (old == a) return;
    a = old;
  }
}

// ============================================================================ labelling
// Tile-local pass.  A wave seeds a row with its runs along W from one ballot (the dominant direction costs no atomic), the
// other backward neighbours inside the tile are united in LDS, and every voxel writes the GLOBAL index of its local root
// (-1 for background).  A pair (v, n) is left out when (v - 1, n - 1) exists and has the same group on both sides: v - 1 ~ v and
// n - 1 ~ n by their runs, and (v - 1, n - 1) is a pair of the same offset, so inside a solid organ only run starts unite.
template <class G>
__global__ __launch_bounds__(256) void cc_tile_kernel(const G src, int D, int H, int W, int nnb, int tiles_h, int tiles_w,
                                                      int *__restrict__ parent) {
  __shared__ int sgroup[G::LDS];
  __shared__ int lpar[TV];
  __shared__ unsigned short sg[TV];
  src.load(sgroup);
  const int t = blockIdx.x;
  const int d0 = t / (tiles_w * tiles_h) * TD, h0 = t / tiles_w % tiles_h * TH, w0 = t % tiles_w * TW;
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1);
  for (int r = threadIdx.x / WAVE; r < TD * TH; r += 256 / WAVE) {
    const int d = d0 + r / TH, h = h0 + r % TH, w = w0 + lane;
    int g = 0;
    if (d < D && h < H && w < W) g = src.at(((int64_t)d * H + h) * W + w, sgroup);
    const int gp = __shfl_up(g, 1, WAVE);
    const unsigned long long starts = __ballot(lane == 0 || g != gp) & (~0ull >> (WAVE - 1 - lane));
    sg[r * TW + lane] = (unsigned short)g;
    lpar[r * TW + lane] = r * TW + (WAVE - 1 - __clzll(starts));          // the last run start at or below this lane
  }
  __syncthreads();
  for (int v = threadIdx.x; v < TV; v += 256) {
    const int g = sg[v];
    if (!g) continue;
    const int lw = v % TW, lh = v / TW % TH, ld = v / (TW * TH);
    for (int k = 1; k < nnb; ++k) {
      const int nd = ld + CC_OFF[k][0], nh = lh + CC_OFF[k][1], nw = lw + CC_OFF[k][2];
      if (nd < 0 || nh < 0 || nh >= TH || nw < 0 || nw >= TW) continue;
      const int n = (nd * TH + nh) * TW + nw;
      if (sg[n] != g) continue;
      if (lw > 0 && nw > 0 && sg[v - 1] == g && sg[n - 1] == g) continue;
      lds_union(lpar, v, n);
    }
  }
  __syncthreads();
  for (int v = threadIdx.x; v < TV; v += 256) {
    const int d = d0 + v / (TW * TH), h = h0 + v / TW % TH, w = w0 + v % TW;
    if (d >= D || h >= H || w >= W) continue;
    int root = -1;
    if (sg[v]) {
      const int r = lds_find(lpar, v);
      root = (int)(((int64_t)(d0 + r / (TW * TH)) * H + (h0 + r / TW % TH)) * W + (w0 + r % TW));
    }
    parent[((int64_t)d * H + h) * W + w] = root;
  }
}

// Border pass: the pairs (voxel, backward neighbour) that lie in two tiles, united in the global forest.  A wave takes a row
// (d, h) at a time.  A pair leaves the tile through a lower face or, with a diagonal offset, through the upper H or W face: in a
// row on such a D or H face every voxel is looked at, in the other rows only the voxels on the W faces, two in 64.
template <class G>
__global__ __launch_bounds__(256) void cc_border_kernel(const G src, int D, int H, int W, int nnb, int *parent) {
  __shared__ int sgroup[G::LDS];
  src.load(sgroup);
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1), faces = 2 * cdiv(W, TW);
  const int64_t rows = (int64_t)D * H;
  for (int64_t row = blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE; row < rows; row += gridDim.x * (256 / WAVE)) {
    const int d = (int)(row / H), h = (int)(row % H);
    const bool whole = d % TD == 0 || h % TH == 0 || (nnb > 3 && h % TH == TH - 1);
    for (int j = lane; j < (whole ? W : faces); j += WAVE) {
      const int w = whole ? j : (j >> 1) * TW + (j & 1) * (TW - 1);
      if (w >= W || (!whole && (j & 1) && nnb == 3)) continue;
      const int64_t i = row * W + w;
      const int g = src.at(i, sgroup);
      if (!g) continue;
      for (int k = 0; k < nnb; ++k) {
        const int dd = CC_OFF[k][0], dh = CC_OFF[k][1], dw = CC_OFF[k][2];
        const int nd = d + dd, nh = h + dh, nw = w + dw;
        if (nd < 0 || nh < 0 || nh >= H || nw < 0 || nw >= W) continue;
        if (nd / TD == d / TD && nh / TH == h / TH && nw / TW == w / TW) continue;    // the tile pass had this pair
        const int64_t n = i + ((int64_t)dd * H + dh) * W + dw;
        if (src.at(n, sgroup) != g) continue;
        if (k > 0 && w > 0 && nw > 0 && src.at(i - 1, sgroup) == g && src.at(n - 1, sgroup) == g) continue;
        glb_union(parent, (int)i, (int)n);
      }
    }
  }
}

// Its own launch: everything the border pass stored is visible, and parent[] is only read.
__global__ __launch_bounds__(256) void cc_flatten_kernel(const int *__restrict__ parent, int64_t total, int *__restrict__ cc) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int p = parent[i], q;
    if (p >= 0)
      while ((q = parent[p]) != p) p = q;
    cc[i] = p + 1;
  }
}

// ============================================================================ sizes
// A wave walks spans of SZ_CHUNKS * 64 consecutive voxels and carries ONE component (cur, cnt), wave uniform, along: the lanes
// of a chunk that belong to it are counted by a ballot, wherever they sit, and added once when the wave is done or takes up another
// component (when a chunk has none of its voxels left).  The other voxels go by runs, one add per run from its first lane.  A
// solid organ is an add per wave, and so is the one component that fills most of a noise volume and whose runs are two voxels long.
constexpr int SZ_CHUNKS = 32;

__global__ __launch_bounds__(256) void cc_sizes_kernel(const int *__restrict__ cc, int64_t n, int *__restrict__ size) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t nspan = cdiv64(n, WAVE * SZ_CHUNKS), nwave = (int64_t)gridDim.x * (256 / WAVE);
  int cur = 0, cnt = 0;
  for (int64_t s = (int64_t)blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE; s < nspan; s += nwave) {
    for (int c = 0; c < SZ_CHUNKS; ++c) {
      const int64_t i = (s * SZ_CHUNKS + c) * WAVE + lane;
      const int v = i < n ? cc[i] : 0;
      unsigned long long mine = __ballot(v && v == cur);
      if (!mine) {
        const unsigned long long any = __ballot(v != 0);
        if (!any) continue;
        if (lane == 0 && cur) atomicAdd(&size[cur - 1], cnt);
        cur = __shfl(v, WAVE - 1 - __clzll(any), WAVE);                   // take up the component of the chunk's last voxel
        cnt = 0;
        mine = __ballot(v == cur);
      }
      cnt += __popcll(mine);
      const int u = v == cur ? 0 : v;
      int prev = __shfl_up(u, 1, WAVE);
      if (lane == 0) prev = 0;
      const unsigned long long heads = __ballot(u != prev);
      if (u && ((heads >> lane) & 1)) {
        const unsigned long long above = heads & ~((2ull << lane) - 1);   // lane 63: 2 << 63 wraps to 0, nothing is above
        atomicAdd(&size[u - 1], (above ? __ffsll(above) - 1 : WAVE) - lane);
      }
    }
  }
  if (lane == 0 && cur) atomicAdd(&size[cur - 1], cnt);
}

// ============================================================================ selection and filter
// winner[c] = max over the components of group c of (size << 32) | ~first index: the largest, ties to the smaller index
__global__ __launch_bounds__(256) void cc_winner_kernel(const int64_t *__restrict__ map, const int *__restrict__ group, int ntab,
                                                        const int *__restrict__ size, int64_t n, unsigned long long *winner) {
  __shared__ int sgroup[CC_MAXTAB];
  load_groups(sgroup, group, ntab);
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int s = size[i];
    if (s <= 0) continue;
    const int g = group_of(map[i], sgroup, ntab);
    if (g) atomicMax(&winner[g], ((unsigned long long)s << 32) | (unsigned)~(unsigned)i);
  }
}

__global__ __launch_bounds__(256) void cc_filter_kernel(const int64_t *__restrict__ map, const int *__restrict__ group, int ntab,
                                                        const int *__restrict__ cc, const int *__restrict__ size, int64_t n,
                                                        int keep_largest, int min_voxels, int64_t background,
                                                        const unsigned long long *__restrict__ winner, int64_t *__restrict__ out,
                                                        unsigned long long *removed) {
  __shared__ int sgroup[CC_MAXTAB];
  __shared__ int srem[CC_MAXTAB];
  load_groups(sgroup, group, ntab);
  for (int i = threadIdx.x; i < ntab; i += blockDim.x) srem[i] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t m = map[i];
    const int g = group_of(m, sgroup, ntab), r = cc[i] - 1;
    if (g && r >= 0) {
      const bool keep = size[r] >= min_voxels && (!keep_largest || (int)~(unsigned)winner[g] == r);
      if (!keep) {
        m = background;
        atomicAdd(&srem[g], 1);
      }
    }
    out[i] = m;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < ntab; c += blockDim.x)
    if (srem[c]) atomicAdd(&removed[c], (unsigned long long)srem[c]);
}

__global__ void cc_clear_kernel(unsigned long long *winner, unsigned long long *removed, int ntab) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ntab; i += gridDim.x * blockDim.x) winner[i] = 0, removed[i] = 0;
}

// the forest of the components of `src` in parent[]: the tile pass, then the border pass
template <class G>
int cc_forest(const G src, int D, int H, int W, int connectivity, int *parent, hipStream_t st) {
  const int nnb = connectivity == 6 ? 3 : connectivity == 18 ? 9 : 13;
  const int tiles_d = cdiv(D, TD), tiles_h = cdiv(H, TH), tiles_w = cdiv(W, TW);
  hipLaunchKernelGGL(cc_tile_kernel<G>, dim3((unsigned)(tiles_d * tiles_h * tiles_w)), dim3(256), 0, st, src, D, H, W, nnb, tiles_h,
                     tiles_w, parent);
  DG_CHECK_LAUNCH("cc_tile_kernel");
  hipLaunchKernelGGL(cc_border_kernel<G>, dim3(gs_blocks((int64_t)D * H * WAVE, 1 << 16)), dim3(256), 0, st, src, D, H, W, nnb, parent);
  DG_CHECK_LAUNCH("cc_border_kernel");
  return DGTTA_OK;
}

// ============================================================================ hole filling
// A voxel outside the mask is ENCLOSED iff its component of the complement has no voxel on any of the six faces of the volume.
// parent[] is the forest of the complement as the border pass left it (read only from here on, each in a launch of its own).
__device__ __forceinline__ int hf_root(const int *__restrict__ parent, int64_t i) {
  int p = parent[i], q;
  while ((q = parent[p]) != p) p = q;
  return p;
}

__global__ void hf_clear_kernel(unsigned long long *n_filled, int *box) {
  if (threadIdx.x == 0) *n_filled = 0;
  if (box && threadIdx.x < 6) box[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : -1;
}

// open[root] = 1 for every component of the complement with a voxel on a face.  A wave takes a row (d, h): all of it when the row
// lies on a D or H face, else its two ends.  Every writer stores the same byte.
__global__ __launch_bounds__(256) void hf_mark_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ parent, int D, int H, int W,
                                                      uint8_t *open) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t rows = (int64_t)D * H;
  for (int64_t row = blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE; row < rows; row += gridDim.x * (256 / WAVE)) {
    const int d = (int)(row / H), h = (int)(row % H);
    const bool whole = d == 0 || d == D - 1 || h == 0 || h == H - 1;
    for (int j = lane; j < (whole ? W : 2); j += WAVE) {
      const int64_t i = row * W + (whole ? j : j * (W - 1));
      if (!mask[i]) open[hf_root(parent, i)] = 1;
    }
  }
}

// out = mask plus its enclosed voxels; n_filled counts the enclosed ones, box (optional) is the inclusive bounding box of out.
// A wave takes a row (d, h) at a time, so the box of what it wrote is wave uniform: the ends along W come from a ballot.
__global__ __launch_bounds__(256) void hf_fill_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ parent,
                                                      const uint8_t *__restrict__ open, int D, int H, int W, uint8_t *__restrict__ out,
                                                      unsigned long long *n_filled, int *box) {
  __shared__ int sbox[6];
  __shared__ unsigned scount;
  if (threadIdx.x < 6) sbox[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : -1;
  if (threadIdx.x == 0) scount = 0;
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t rows = (int64_t)D * H;
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
  unsigned count = 0;
  for (int64_t row = blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE; row < rows; row += gridDim.x * (256 / WAVE)) {
    const int d = (int)(row / H), h = (int)(row % H);
    int wlo = INT_MAX, whi = -1;
    for (int w0 = 0; w0 < W; w0 += WAVE) {
      const int w = w0 + lane;
      bool member = false, enclosed = false;
      if (w < W) {
        const int64_t i = row * W + w;
        member = mask[i] != 0;
        enclosed = !member && !open[hf_root(parent, i)];
        out[i] = member || enclosed;
      }
      count += __popcll(__ballot(enclosed));
      const unsigned long long set = __ballot(member || enclosed);
      if (set) wlo = min(wlo, w0 + __ffsll((long long)set) - 1), whi = w0 + WAVE - 1 - __clzll(set);
    }
    if (whi >= 0) {
      lo[0] = min(lo[0], d), hi[0] = max(hi[0], d);
      lo[1] = min(lo[1], h), hi[1] = max(hi[1], h);
      lo[2] = min(lo[2], wlo), hi[2] = max(hi[2], whi);
    }
  }
  if (lane == 0) {
    atomicAdd(&scount, count);
    if (hi[0] >= 0)
      for (int k = 0; k < 3; ++k) atomicMin(&sbox[k], lo[k]), atomicMax(&sbox[3 + k], hi[k]);
  }
  __syncthreads();
  if (threadIdx.x == 0 && scount) atomicAdd(n_filled, (unsigned long long)scount);
  if (box && threadIdx.x < 3 && sbox[3] >= 0) atomicMin(&box[threadIdx.x], sbox[threadIdx.x]), atomicMax(&box[3 + threadIdx.x], sbox[3 + threadIdx.x]);
}

// mask = 1 where group[map] != 0 (labels and entries outside the table count as 0), inside the crop box
__global__ __launch_bounds__(256) void hf_member_kernel(const int64_t *__restrict__ map, const int *__restrict__ group, int ntab, int H, int W,
                                                        int d0, int h0, int w0, int ch, int cw, int64_t total, uint8_t *__restrict__ mask) {
  __shared__ int sgroup[CC_MAXTAB];
  load_groups(sgroup, group, ntab);
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cw;
    const int d = d0 + (int)(r / ch), h = h0 + (int)(r % ch), w = w0 + (int)(i % cw);
    mask[i] = group_of(map[((int64_t)d * H + h) * W + w], sgroup, ntab) != 0;
  }
}

// inside the crop box, a voxel that `filled` has and `mask` has not (an enclosed one) and whose value is `background` becomes `label`
__global__ __launch_bounds__(256) void hf_apply_kernel(int64_t *__restrict__ map, const uint8_t *__restrict__ mask,
                                                       const uint8_t *__restrict__ filled, int H, int W, int d0, int h0, int w0, int ch, int cw,
                                                       int64_t total, int64_t background, int64_t label, unsigned long long *count) {
  __shared__ unsigned scount;
  if (threadIdx.x == 0) scount = 0;
  __syncthreads();
  unsigned mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (!filled[i] || mask[i]) continue;
    const int64_t r = i / cw;
    const int d = d0 + (int)(r / ch), h = h0 + (int)(r % ch), w = w0 + (int)(i % cw);
    int64_t *m = map + ((int64_t)d * H + h) * W + w;
    if (*m == background) *m = label, ++mine;
  }
  if (mine) atomicAdd(&scount, mine);
  __syncthreads();
  if (threadIdx.x == 0 && scount) atomicAdd(count, (unsigned long long)scount);
}

// ============================================================================ non-zero mask of the crop
// mask[i] = OR over c of (data[c][i] != 0), IEEE: NaN counts as non-zero and -0.0 as zero.  Four voxels per thread (one 16-byte
// load per channel, one 4-byte store) where n and the pointers allow it, else one.
template <bool VEC>
__global__ __launch_bounds__(256) void nonzero_mask_kernel(const float *__restrict__ data, int C, int64_t n, uint8_t *__restrict__ mask) {
  const int64_t items = VEC ? n / 4 : n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (VEC) {
      unsigned any = 0;
      for (int c = 0; c < C; ++c) {
        const float4 x = *(const float4 *)(data + c * n + i * 4);
        any |= (unsigned)(x.x != 0.f) | (unsigned)(x.y != 0.f) << 8 | (unsigned)(x.z != 0.f) << 16 | (unsigned)(x.w != 0.f) << 24;
      }
      *(unsigned *)(mask + i * 4) = any;
    } else {
      bool any = false;
      for (int c = 0; c < C; ++c) any |= data[c * n + i] != 0.f;
      mask[i] = any;
    }
  }
}

}  // namespace

extern "C" size_t dgtta_cc_ws_bytes(int D, int H, int W) {
  if (D <= 0 || H <= 0 || W <= 0) return 0;
  const size_t forest = align_up((size_t)D * (size_t)H * (size_t)W * sizeof(int), 256), table = CC_MAXTAB * sizeof(unsigned long long);
  return forest > table ? forest : table;
}

extern "C" int dgtta_cc_label(const int64_t *map, const int *group, int ntab, int D, int H, int W, int connectivity, int *cc, void *ws,
                              size_t ws_bytes, void *stream) {
  DG_REQUIRE(map && group && cc && ws && D > 0 && H > 0 && W > 0 && ntab > 0, DGTTA_ERR_BADARG, "cc_label: bad args");
  DG_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, DGTTA_ERR_BADARG, "cc_label: connectivity %d (6, 18 or 26)",
             connectivity);
  DG_REQUIRE(ntab <= CC_MAXTAB, DGTTA_ERR_UNSUPPORTED, "cc_label: group table of %d entries (at most %d)", ntab, CC_MAXTAB);
  const int64_t total = (int64_t)D * H * W;
  DG_REQUIRE(total < INT_MAX, DGTTA_ERR_UNSUPPORTED, "cc_label: %d x %d x %d voxels (fewer than 2^31 - 1: components are named by int32)",
             D, H, W);
  DG_REQUIRE(ws_bytes >= dgtta_cc_ws_bytes(D, H, W), DGTTA_ERR_WORKSPACE, "cc_label: workspace %zu < %zu", ws_bytes,
             dgtta_cc_ws_bytes(D, H, W));
  DG_REQUIRE(((uintptr_t)ws & 3) == 0, DGTTA_ERR_BADARG, "cc_label: workspace must be 4-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  int *parent = (int *)ws;
  const int rc = cc_forest(MapGroups{map, group, ntab}, D, H, W, connectivity, parent, st);
  if (rc != DGTTA_OK) return rc;
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(gs_blocks(total, 1 << 16)), dim3(256), 0, st, parent, total, cc);
  DG_CHECK_LAUNCH("cc_flatten_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_cc_sizes(const int *cc, int64_t n, int *size, void *stream) {
  DG_REQUIRE(cc && size && n > 0, DGTTA_ERR_BADARG, "cc_sizes: bad args");
  DG_REQUIRE(n < INT_MAX, DGTTA_ERR_UNSUPPORTED, "cc_sizes: %lld voxels (fewer than 2^31 - 1)", (long long)n);
  const hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(size, 0, (size_t)n * sizeof(int), st);
  DG_REQUIRE(e == hipSuccess, DGTTA_ERR_LAUNCH, "cc_sizes: memset failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(cc_sizes_kernel, dim3(gs_blocks(cdiv64(n, SZ_CHUNKS), 1 << 16)), dim3(256), 0, st, cc, n, size);
  DG_CHECK_LAUNCH("cc_sizes_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_cc_filter(const int64_t *map, const int *group, int ntab, const int *cc, const int *size, int64_t n, int keep_largest,
                               int min_voxels, int64_t background, int64_t *out, int64_t *removed, void *ws, size_t ws_bytes,
                               void *stream) {
  DG_REQUIRE(map && group && cc && size && out && removed && ws && n > 0 && ntab > 0, DGTTA_ERR_BADARG, "cc_filter: bad args");
  DG_REQUIRE(ntab <= CC_MAXTAB, DGTTA_ERR_UNSUPPORTED, "cc_filter: group table of %d entries (at most %d)", ntab, CC_MAXTAB);
  DG_REQUIRE(n < INT_MAX, DGTTA_ERR_UNSUPPORTED, "cc_filter: %lld voxels (fewer than 2^31 - 1)", (long long)n);
  DG_REQUIRE(ws_bytes >= (size_t)ntab * sizeof(unsigned long long), DGTTA_ERR_WORKSPACE, "cc_filter: workspace %zu < %zu", ws_bytes,
             (size_t)ntab * sizeof(unsigned long long));
  DG_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)removed & 7) == 0, DGTTA_ERR_BADARG, "cc_filter: ws and removed must be 8-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long *winner = (unsigned long long *)ws;
  hipLaunchKernelGGL(cc_clear_kernel, dim3(cdiv(ntab, 256)), dim3(256), 0, st, winner, (unsigned long long *)removed, ntab);
  DG_CHECK_LAUNCH("cc_clear_kernel");
  if (keep_largest) {
    hipLaunchKernelGGL(cc_winner_kernel, dim3(gs_blocks(n, 1 << 16)), dim3(256), 0, st, map, group, ntab, size, n, winner);
    DG_CHECK_LAUNCH("cc_winner_kernel");
  }
  hipLaunchKernelGGL(cc_filter_kernel, dim3(gs_blocks(n, 4096)), dim3(256), 0, st, map, group, ntab, cc, size, n, keep_largest, min_voxels,
                     background, winner, out, (unsigned long long *)removed);
  DG_CHECK_LAUNCH("cc_filter_kernel");
  return DGTTA_OK;
}

// workspace of holes_fill: the forest (int32 per voxel), then the open flag (a byte per voxel)
static size_t holes_forest_bytes(int D, int H, int W) { return align_up((size_t)D * (size_t)H * (size_t)W * sizeof(int), 256); }

extern "C" size_t dgtta_holes_ws_bytes(int D, int H, int W) {
  if (D <= 0 || H <= 0 || W <= 0) return 0;
  return holes_forest_bytes(D, H, W) + align_up((size_t)D * (size_t)H * (size_t)W, 256);
}

extern "C" int dgtta_holes_fill(const uint8_t *mask, int D, int H, int W, int connectivity, uint8_t *out, int64_t *n_filled, int *box,
                                void *ws, size_t ws_bytes, void *stream) {
  DG_REQUIRE(mask && out && n_filled && ws && D > 0 && H > 0 && W > 0, DGTTA_ERR_BADARG, "holes_fill: bad args");
  DG_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, DGTTA_ERR_BADARG, "holes_fill: connectivity %d (6, 18 or 26)",
             connectivity);
  const int64_t total = (int64_t)D * H * W;
  DG_REQUIRE(total < INT_MAX, DGTTA_ERR_UNSUPPORTED, "holes_fill: %d x %d x %d voxels (fewer than 2^31 - 1: components are named by int32)",
             D, H, W);
  DG_REQUIRE(ws_bytes >= dgtta_holes_ws_bytes(D, H, W), DGTTA_ERR_WORKSPACE, "holes_fill: workspace %zu < %zu", ws_bytes,
             dgtta_holes_ws_bytes(D, H, W));
  DG_REQUIRE(((uintptr_t)ws & 3) == 0 && ((uintptr_t)n_filled & 7) == 0 && ((uintptr_t)box & 3) == 0, DGTTA_ERR_BADARG,
             "holes_fill: ws and box must be 4-byte aligned, n_filled 8-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  int *parent = (int *)ws;
  uint8_t *open = (uint8_t *)ws + holes_forest_bytes(D, H, W);
  const hipError_t e = hipMemsetAsync(open, 0, (size_t)total, st);
  DG_REQUIRE(e == hipSuccess, DGTTA_ERR_LAUNCH, "holes_fill: memset failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(hf_clear_kernel, dim3(1), dim3(WAVE), 0, st, (unsigned long long *)n_filled, box);
  DG_CHECK_LAUNCH("hf_clear_kernel");
  const int rc = cc_forest(MaskComplement{mask}, D, H, W, connectivity, parent, st);
  if (rc != DGTTA_OK) return rc;
  const int row_blocks = gs_blocks((int64_t)D * H * WAVE, 1 << 16);
  hipLaunchKernelGGL(hf_mark_kernel, dim3(row_blocks), dim3(256), 0, st, mask, parent, D, H, W, open);
  DG_CHECK_LAUNCH("hf_mark_kernel");
  hipLaunchKernelGGL(hf_fill_kernel, dim3(row_blocks), dim3(256), 0, st, mask, parent, open, D, H, W, out, (unsigned long long *)n_filled, box);
  DG_CHECK_LAUNCH("hf_fill_kernel");
  return DGTTA_OK;
}

// the crop box (d0, h0, w0, cd, ch, cw) must lie inside the volume
static bool holes_box_ok(int D, int H, int W, int d0, int h0, int w0, int cd, int ch, int cw) {
  return D > 0 && H > 0 && W > 0 && d0 >= 0 && h0 >= 0 && w0 >= 0 && cd > 0 && ch > 0 && cw > 0 && cd <= D - d0 && ch <= H - h0 && cw <= W - w0;
}

extern "C" int dgtta_holes_member(const int64_t *map, int D, int H, int W, const int *group, int ntab, int d0, int h0, int w0, int cd,
                                  int ch, int cw, uint8_t *mask, void *stream) {
  DG_REQUIRE(map && group && mask && ntab > 0, DGTTA_ERR_BADARG, "holes_member: bad args");
  DG_REQUIRE(ntab <= CC_MAXTAB, DGTTA_ERR_UNSUPPORTED, "holes_member: group table of %d entries (at most %d)", ntab, CC_MAXTAB);
  DG_REQUIRE(holes_box_ok(D, H, W, d0, h0, w0, cd, ch, cw), DGTTA_ERR_BADARG, "holes_member: box (%d, %d, %d) + (%d, %d, %d) outside %d x %d x %d",
             d0, h0, w0, cd, ch, cw, D, H, W);
  const int64_t total = (int64_t)cd * ch * cw;
  hipLaunchKernelGGL(hf_member_kernel, dim3(gs_blocks(total, 4096)), dim3(256), 0, (hipStream_t)stream, map, group, ntab, H, W, d0, h0, w0,
                     ch, cw, total, mask);
  DG_CHECK_LAUNCH("hf_member_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_holes_apply(int64_t *map, int D, int H, int W, const uint8_t *mask, const uint8_t *filled, int d0, int h0, int w0,
                                 int cd, int ch, int cw, int64_t background, int64_t label, int64_t *count, void *stream) {
  DG_REQUIRE(map && mask && filled && count, DGTTA_ERR_BADARG, "holes_apply: bad args");
  DG_REQUIRE(((uintptr_t)count & 7) == 0, DGTTA_ERR_BADARG, "holes_apply: count must be 8-byte aligned");
  DG_REQUIRE(holes_box_ok(D, H, W, d0, h0, w0, cd, ch, cw), DGTTA_ERR_BADARG, "holes_apply: box (%d, %d, %d) + (%d, %d, %d) outside %d x %d x %d",
             d0, h0, w0, cd, ch, cw, D, H, W);
  const hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), st);
  DG_REQUIRE(e == hipSuccess, DGTTA_ERR_LAUNCH, "holes_apply: memset failed: %s", hipGetErrorString(e));
  const int64_t total = (int64_t)cd * ch * cw;
  hipLaunchKernelGGL(hf_apply_kernel, dim3(gs_blocks(total, 4096)), dim3(256), 0, st, map, mask, filled, H, W, d0, h0, w0, ch, cw, total,
                     background, label, (unsigned long long *)count);
  DG_CHECK_LAUNCH("hf_apply_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_nonzero_mask(const float *data, int C, int64_t n, uint8_t *mask, void *stream) {
  DG_REQUIRE(data && mask && C > 0 && n > 0, DGTTA_ERR_BADARG, "nonzero_mask: bad args");
  DG_REQUIRE(((uintptr_t)data & 3) == 0, DGTTA_ERR_BADARG, "nonzero_mask: data must be 4-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  if (n % 4 == 0 && ((uintptr_t)data & 15) == 0 && ((uintptr_t)mask & 3) == 0)
    hipLaunchKernelGGL(nonzero_mask_kernel<true>, dim3(gs_blocks(n / 4, 1 << 16)), dim3(256), 0, st, data, C, n, mask);
  else
    hipLaunchKernelGGL(nonzero_mask_kernel<false>, dim3(gs_blocks(n, 1 << 16)), dim3(256), 0, st, data, C, n, mask);
  DG_CHECK_LAUNCH("nonzero_mask_kernel");
  return DGTTA_OK;
}
