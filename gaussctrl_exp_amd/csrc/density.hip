// density.hip -- splatfacto's density control (refinement statistics, cull / split / duplicate)
// for the Gaussian parameter groups on gfx950.
//
// nerfstudio's SplatfactoModel, which the reference trains through with its refinement defaults
// (GaussCtrlModelConfig, gc_config.py), folds xys.grad and radii into three per-Gaussian
// statistics after every iteration (after_train) and, every refine_every steps, culls, splits
// and duplicates Gaussians and edits the Adam state to match (refinement_after).  In torch ops
// the first is ~10 small kernels with a host sync per boolean-mask index, the second a boolean
// index + cat over 18 tensors.  Here:
//
//   gsplat_density_accumulate  one launch per step: reads v_xy (8 B) and radii (4 B), reads and
//                              writes the three statistics (24 B): 36 B per Gaussian, no sync.
//   gsplat_density_plan        the per-row predicates from the raw parameters, the statistics
//                              and the scalar config; exclusive scans of the three per-row
//                              counters (kept original, kept split parent, kept duplicate) by
//                              reduce-then-scan in three launches (per-block sums, one block
//                              over the sums, per-row offsets) -- no workgroup waits for
//                              another; totals {K, S, Dn, new_N} for the host's one read.
//   gsplat_density_apply       the output rows' source map (one scatter launch), then ONE
//                              gather launch over the flattened elements of all 18 outputs
//                              (6 parameters, 12 Adam moments): survivors copied bit for bit,
//                              split children computed, duplicates copied, zero moments for new
//                              rows, the optional opacity reset.  Four consecutive output
//                              elements per thread, one 16-byte store: ~2 x 708 B per output
//                              row at SH degree 3 (read + write), the floor of the edit.
//
// The semantics are the maintainers' recollection of splatfacto 1.0.0: the
// statistics' first-call rule (vis_counts = 1 for every row), avg = grad_norm / vis_counts *
// 0.5 * max(H, W), children = R(q / |q|) (exp(scales) * z) + mean with scales
// log(exp(scales) / 1.6), the cull of the concatenated set.
#include <math.h>

#include "common.h"

namespace gs {
namespace {

constexpr int DN_TPB = GSPLAT_DENSITY_PLAN_ROWS;  // rows per block of the row kernels (256)
static_assert(DN_TPB == 256, "pack_flags holds a block's counters in 10 bits each");
constexpr int DN_SCAN_TPB = 1024;    // the one block that scans the per-block sums
constexpr int DN_VEC = 4;            // output elements per thread of the gather
constexpr int DN_MAX_SAMPLES = 16;   // n_split_samples bound (splatfacto: 2)
constexpr int DN_SEGS = 18;
typedef float f4 __attribute__((ext_vector_type(4)));

enum { FLAG_KEEP = 1, FLAG_SPLIT = 2, FLAG_DUP = 4 };
enum { SEG_COPY = 0, SEG_MEANS, SEG_SCALES, SEG_OPACITY, SEG_MOMENT, SEG_OPACITY_MOMENT };

// ---- statistics ---------------------------------------------------------------------------
__global__ __launch_bounds__(DN_TPB) void density_accumulate_kernel(
    int n, const float *__restrict__ v_xy, const int *__restrict__ radii, float max_dim,
    int first, float *__restrict__ grad_norm, float *__restrict__ vis_counts,
    float *__restrict__ max_2dsize) {
  const int i = blockIdx.x * DN_TPB + threadIdx.x;
  if (i >= n) return;
  const float2 v = reinterpret_cast<const float2 *>(v_xy)[i];
  const int r = radii[i];
  const float g = sqrtf(v.x * v.x + v.y * v.y);
  const bool vis = r > 0;
  float m;
  if (first) {  // splatfacto's first call: every row, visible or not
    grad_norm[i] = g;
    vis_counts[i] = 1.f;
    m = 0.f;
  } else {
    m = max_2dsize[i];
    if (vis) {
      vis_counts[i] = vis_counts[i] + 1.f;
      grad_norm[i] = grad_norm[i] + g;
    }
  }
  if (vis) m = fmaxf(m, (float)r / max_dim);
  if (first || vis) max_2dsize[i] = m;
}

// ---- plan ---------------------------------------------------------------------------------
struct PlanCfg {
  int mode;  // 0 nothing deleted, 1 densify + cull, 2 cull only
  int toobig_on, screen_on;
  float max_dim;
  float cull_alpha, cull_scale, cull_screen, grad_thresh, size_thresh, split_screen;
};

// Exclusive scan of one int per thread over the block (blockDim.x a multiple of 64, at most
// 1024); `total` = the block's sum.  lds: 16 ints.
__device__ __forceinline__ int block_exclusive_scan(int v, int *lds, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
  for (int w = 0; w < waves; ++w) {
    const int t = lds[w];
    if (w < wave) base += t;
    total += t;
  }
  __syncthreads();  // (lds is free for the next scan)
  return base + inc - v;
}

__device__ __forceinline__ int row_flags(int i, const PlanCfg &c, const float *scales,
                                         const float *opacities, const float *grad_norm,
                                         const float *vis_counts, const float *max_2dsize) {
  if (c.mode == 0) return FLAG_KEEP;
  const float e0 = expf(scales[3 * (long long)i]), e1 = expf(scales[3 * (long long)i + 1]),
              e2 = expf(scales[3 * (long long)i + 2]);
  const float size = fmaxf(fmaxf(e0, e1), e2);
  const float sig = 1.f / (1.f + expf(-opacities[i]));
  const bool low = sig < c.cull_alpha;
  const bool big_scale = c.toobig_on && size > c.cull_scale;
  if (c.mode == 2) return (low || big_scale) ? 0 : FLAG_KEEP;
  const float m2d = c.screen_on ? max_2dsize[i] : 0.f;
  const float avg = (grad_norm[i] / vis_counts[i]) * 0.5f * c.max_dim;
  const bool high = avg > c.grad_thresh;
  const bool split = (size > c.size_thresh || (c.screen_on && m2d > c.split_screen)) && high;
  const bool dup = size <= c.size_thresh && high;
  const bool big_screen = c.toobig_on && c.screen_on && m2d > c.cull_screen;
  // the children's cull reads their new scales, log(exp(scales) / 1.6)
  const float child = fmaxf(fmaxf(expf(logf(e0 / 1.6f)), expf(logf(e1 / 1.6f))),
                            expf(logf(e2 / 1.6f)));
  const bool child_big = c.toobig_on && child > c.cull_scale;
  int f = 0;
  if (!(split || low || big_scale || big_screen)) f |= FLAG_KEEP;
  if (split && !(low || child_big)) f |= FLAG_SPLIT;
  if (dup && !(low || big_scale)) f |= FLAG_DUP;
  return f;
}

// the three 0/1 counters of a row in one int (a block sums at most 256 of each: 10 bits)
__device__ __forceinline__ int pack_flags(int f) {
  return (f & FLAG_KEEP ? 1 : 0) | (f & FLAG_SPLIT ? 1 << 10 : 0) | (f & FLAG_DUP ? 1 << 20 : 0);
}

__global__ __launch_bounds__(DN_TPB) void density_flags_kernel(
    int n, PlanCfg c, const float *__restrict__ scales, const float *__restrict__ opacities,
    const float *__restrict__ grad_norm, const float *__restrict__ vis_counts,
    const float *__restrict__ max_2dsize, int *__restrict__ flags, int *__restrict__ partials) {
  __shared__ int lds[16];
  const int i = blockIdx.x * DN_TPB + threadIdx.x;
  int f = 0;
  if (i < n) {
    f = row_flags(i, c, scales, opacities, grad_norm, vis_counts, max_2dsize);
    flags[i] = f;
  }
  int total;
  block_exclusive_scan(pack_flags(f), lds, total);
  if (threadIdx.x == 0) {
    partials[3 * blockIdx.x] = total & 1023;
    partials[3 * blockIdx.x + 1] = (total >> 10) & 1023;
    partials[3 * blockIdx.x + 2] = (total >> 20) & 1023;
  }
}

// One block: the per-block sums [nb][3] -> their exclusive prefixes (in place) and the totals.
__global__ __launch_bounds__(DN_SCAN_TPB) void density_scan_partials_kernel(
    int nb, int n_split_samples, int *__restrict__ partials, int *__restrict__ totals) {
  __shared__ int lds[16];
  const int chunk = (nb + DN_SCAN_TPB - 1) / DN_SCAN_TPB;
  const int b0 = min((int)threadIdx.x * chunk, nb), b1 = min(b0 + chunk, nb);
  int sum[3] = {0, 0, 0};
  for (int b = b0; b < b1; ++b)
    for (int k = 0; k < 3; ++k) sum[k] += partials[3 * b + k];
  int grand[3];
  for (int k = 0; k < 3; ++k) {
    int run = block_exclusive_scan(sum[k], lds, grand[k]);
    for (int b = b0; b < b1; ++b) {
      const int t = partials[3 * b + k];
      partials[3 * b + k] = run;
      run += t;
    }
  }
  if (threadIdx.x == 0) {
    totals[0] = grand[0];
    totals[1] = grand[1];
    totals[2] = grand[2];
    totals[3] = grand[0] + n_split_samples * grand[1] + grand[2];
  }
}

__global__ __launch_bounds__(DN_TPB) void density_offsets_kernel(
    int n, const int *__restrict__ flags, const int *__restrict__ partials,
    int *__restrict__ off_keep, int *__restrict__ off_split, int *__restrict__ off_dup) {
  __shared__ int lds[16];
  const int i = blockIdx.x * DN_TPB + threadIdx.x;
  const int f = i < n ? flags[i] : 0;
  int total;
  const int ex = block_exclusive_scan(pack_flags(f), lds, total);
  if (i >= n) return;
  off_keep[i] = partials[3 * blockIdx.x] + (ex & 1023);
  off_split[i] = partials[3 * blockIdx.x + 1] + ((ex >> 10) & 1023);
  off_dup[i] = partials[3 * blockIdx.x + 2] + ((ex >> 20) & 1023);
}

struct PlanView {
  int *totals, *flags, *off_keep, *off_split, *off_dup, *partials;
  int nb;
  size_t bytes;
};

PlanView plan_view(void *plan, int n) {
  PlanView v;
  int *p = (int *)plan;
  v.nb = (int)cdiv(n, DN_TPB);
  v.totals = p;
  v.flags = p + 4;
  v.off_keep = v.flags + n;
  v.off_split = v.off_keep + n;
  v.off_dup = v.off_split + n;
  v.partials = v.off_dup + n;
  v.bytes = sizeof(int) * (size_t)GSPLAT_DENSITY_PLAN_WORDS((size_t)n);
  return v;
}

// ---- apply --------------------------------------------------------------------------------
// Output row j's source row: [0, K) the kept originals, [K + s S, K + (s + 1) S) the children
// of sample s by kept-split-parent rank, [K + ns S, new_N) the duplicates.
__global__ __launch_bounds__(DN_TPB) void density_source_rows_kernel(
    int n, int new_n, int ns, const int *__restrict__ totals, const int *__restrict__ flags,
    const int *__restrict__ off_keep, const int *__restrict__ off_split,
    const int *__restrict__ off_dup, int *__restrict__ src_rows) {
  const int i = blockIdx.x * DN_TPB + threadIdx.x;
  if (i >= n) return;
  const int f = flags[i];
  const long long K = totals[0], S = totals[1];
  if (f & FLAG_KEEP) {
    const long long j = off_keep[i];
    if (j >= 0 && j < new_n) src_rows[j] = i;
  }
  if (f & FLAG_SPLIT)
    for (int s = 0; s < ns; ++s) {
      const long long j = K + s * S + off_split[i];
      if (j >= 0 && j < new_n) src_rows[j] = i;
    }
  if (f & FLAG_DUP) {
    const long long j = K + ns * S + off_dup[i];
    if (j >= 0 && j < new_n) src_rows[j] = i;
  }
}

struct ApplySeg {
  const float *src;
  float *dst;
  int width, kind;
};
struct ApplyTable {
  ApplySeg seg[DN_SEGS];
  long long block0[DN_SEGS + 1];
  int nseg;
  // the children's inputs
  const float *means, *scales, *quats, *z;
};

__device__ __forceinline__ float child_mean(const ApplyTable &t, long long src, int col, int s,
                                            int n) {
  const float *q = t.quats + 4 * src, *sc = t.scales + 3 * src,
              *zz = t.z + 3 * ((long long)s * n + src);
  float w = q[0], x = q[1], y = q[2], z = q[3];
  const float inv = 1.f / sqrtf(w * w + x * x + y * y + z * z);
  w *= inv, x *= inv, y *= inv, z *= inv;
  const float a = expf(sc[0]) * zz[0], b = expf(sc[1]) * zz[1], c = expf(sc[2]) * zz[2];
  float r;
  if (col == 0)
    r = (1.f - 2.f * (y * y + z * z)) * a + 2.f * (x * y - w * z) * b + 2.f * (x * z + w * y) * c;
  else if (col == 1)
    r = 2.f * (x * y + w * z) * a + (1.f - 2.f * (x * x + z * z)) * b + 2.f * (y * z - w * x) * c;
  else
    r = 2.f * (x * z - w * y) * a + 2.f * (y * z + w * x) * b + (1.f - 2.f * (x * x + y * y)) * c;
  return r + t.means[3 * src + col];
}

__global__ __launch_bounds__(DN_TPB) void density_gather_kernel(
    ApplyTable t, int n, int new_n, int ns, const int *__restrict__ totals,
    const int *__restrict__ src_rows, int reset_opacity, float opacity_cap) {
  int s = 0;
  while (s + 1 < t.nseg && (long long)blockIdx.x >= t.block0[s + 1]) ++s;
  const ApplySeg sg = t.seg[s];
  const int W = sg.width;
  // rows the plan produced (a caller's new_n beyond them has no source row: left unwritten)
  const long long rows = min((long long)new_n, (long long)totals[3]);
  const long long K = totals[0], S = totals[1], total = rows * W;
  const long long e0 = (((long long)blockIdx.x - t.block0[s]) * DN_TPB + threadIdx.x) * DN_VEC;
  if (e0 >= total) return;
  long long row = e0 / W;
  int col = (int)(e0 - row * W);
  float out[DN_VEC];
#pragma unroll
  for (int k = 0; k < DN_VEC; ++k) {
    float v = 0.f;
    if (e0 + k < total) {
      const long long src = src_rows[row];
      if (src >= 0 && src < n) {
        const bool survivor = row < K, child = !survivor && row < K + ns * S;
        const float in = sg.src[src * W + col];
        switch (sg.kind) {
          case SEG_MEANS:
            v = child ? child_mean(t, src, col, (int)((row - K) / S), n) : in;
            break;
          case SEG_SCALES:
            v = child ? logf(expf(in) / 1.6f) : in;
            break;
          case SEG_OPACITY:
            v = reset_opacity ? fminf(in, opacity_cap) : in;
            break;
          case SEG_MOMENT:
            v = survivor ? in : 0.f;
            break;
          case SEG_OPACITY_MOMENT:
            v = (survivor && !reset_opacity) ? in : 0.f;
            break;
          default:
            v = in;
        }
      }
    }
    out[k] = v;
    if (++col == W) col = 0, ++row;
  }
  float *dst = sg.dst + e0;
  if (e0 + DN_VEC <= total && (((uintptr_t)dst) & 15) == 0) {
    f4 o;
    o[0] = out[0], o[1] = out[1], o[2] = out[2], o[3] = out[3];
    *reinterpret_cast<f4 *>(dst) = o;
  } else {
    for (int k = 0; k < DN_VEC && e0 + k < total; ++k) dst[k] = out[k];
  }
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" int gsplat_density_accumulate(int num_points, const float *v_xy, const int32_t *radii,
                                         int img_height, int img_width, int first,
                                         float *grad_norm, float *vis_counts, float *max_2dsize,
                                         void *stream) {
  if (num_points < 0 || img_height < 1 || img_width < 1) {
    set_error("density_accumulate: bad sizes (n=%d H=%d W=%d)", num_points, img_height,
              img_width);
    return 1;
  }
  if (num_points == 0) return 0;
  if (!v_xy || !radii || !grad_norm || !vis_counts || !max_2dsize) {
    set_error("density_accumulate: null pointer");
    return 1;
  }
  const float max_dim = (float)(img_height > img_width ? img_height : img_width);
  hipLaunchKernelGGL(density_accumulate_kernel, dim3(cdiv(num_points, DN_TPB)), dim3(DN_TPB), 0,
                     (hipStream_t)stream, num_points, v_xy, (const int *)radii, max_dim, first,
                     grad_norm, vis_counts, max_2dsize);
  return check_launch("density_accumulate");
}

extern "C" int gsplat_density_plan(int num_points, const float *scales, const float *opacities,
                                   const float *grad_norm, const float *vis_counts,
                                   const float *max_2dsize, int mode, int toobig_on,
                                   int screen_on, int n_split_samples, int max_dim,
                                   float cull_alpha_thresh, float cull_scale_thresh,
                                   float cull_screen_size, float densify_grad_thresh,
                                   float densify_size_thresh, float split_screen_size,
                                   int32_t *plan, size_t plan_bytes, void *stream) {
  if (num_points < 0 || mode < 0 || mode > 2 || n_split_samples < 1 ||
      n_split_samples > DN_MAX_SAMPLES || max_dim < 1) {
    set_error("density_plan: bad args (n=%d mode=%d samples=%d max_dim=%d)", num_points, mode,
              n_split_samples, max_dim);
    return 1;
  }
  if ((long long)num_points * (2 + n_split_samples) > 2147483647LL) {
    set_error("density_plan: %d Gaussians x (2 + %d samples) rows exceed int32", num_points,
              n_split_samples);
    return 1;
  }
  const PlanView v = plan_view(plan, num_points);
  if (!plan || plan_bytes < v.bytes) {
    set_error("density_plan: plan buffer too small (%zu < %zu bytes)", plan_bytes, v.bytes);
    return 1;
  }
  if (num_points > 0 &&
      ((mode != 0 && (!scales || !opacities)) ||
       (mode == 1 && (!grad_norm || !vis_counts || (screen_on && !max_2dsize))))) {
    set_error("density_plan: null pointer (mode %d needs its inputs)", mode);
    return 1;
  }
  PlanCfg c;
  c.mode = mode;
  c.toobig_on = toobig_on != 0;
  c.screen_on = screen_on != 0;
  c.max_dim = (float)max_dim;
  c.cull_alpha = cull_alpha_thresh;
  c.cull_scale = cull_scale_thresh;
  c.cull_screen = cull_screen_size;
  c.grad_thresh = densify_grad_thresh;
  c.size_thresh = densify_size_thresh;
  c.split_screen = split_screen_size;
  hipStream_t st = (hipStream_t)stream;
  if (num_points > 0)
    hipLaunchKernelGGL(density_flags_kernel, dim3(v.nb), dim3(DN_TPB), 0, st, num_points, c,
                       scales, opacities, grad_norm, vis_counts, max_2dsize, v.flags, v.partials);
  hipLaunchKernelGGL(density_scan_partials_kernel, dim3(1), dim3(DN_SCAN_TPB), 0, st, v.nb,
                     n_split_samples, v.partials, v.totals);
  if (num_points > 0)
    hipLaunchKernelGGL(density_offsets_kernel, dim3(v.nb), dim3(DN_TPB), 0, st, num_points,
                       v.flags, v.partials, v.off_keep, v.off_split, v.off_dup);
  return check_launch("density_plan");
}

extern "C" int gsplat_density_apply(int num_points, int new_points, int sh_bases,
                                    int n_split_samples, const int32_t *plan, size_t plan_bytes,
                                    const float *const *params, const float *const *exp_avgs,
                                    const float *const *exp_avg_sqs, const float *z,
                                    float *const *out_params, float *const *out_exp_avgs,
                                    float *const *out_exp_avg_sqs, int32_t *src_rows,
                                    int reset_opacity, float opacity_cap, void *stream) {
  if (num_points < 0 || new_points < 0 || n_split_samples < 1 ||
      n_split_samples > DN_MAX_SAMPLES ||
      !(sh_bases == 1 || sh_bases == 4 || sh_bases == 9 || sh_bases == 16 || sh_bases == 25) ||
      (long long)num_points * (2 + n_split_samples) > 2147483647LL ||
      (long long)new_points > (long long)num_points * (2 + n_split_samples)) {
    set_error("density_apply: bad args (n=%d new_n=%d K=%d samples=%d)", num_points, new_points,
              sh_bases, n_split_samples);
    return 1;
  }
  if (num_points == 0 || new_points == 0) return 0;
  const PlanView v = plan_view((void *)plan, num_points);
  if (!plan || plan_bytes < v.bytes || !src_rows || !z || !params || !exp_avgs || !exp_avg_sqs ||
      !out_params || !out_exp_avgs || !out_exp_avg_sqs) {
    set_error("density_apply: null pointer or plan buffer too small");
    return 1;
  }
  // means, scales, quats, opacities, features_dc, features_rest (scene.PARAM_NAMES)
  const int width[6] = {3, 3, 4, 1, 3, 3 * (sh_bases - 1)};
  const int kind[6] = {SEG_MEANS, SEG_SCALES, SEG_COPY, SEG_OPACITY, SEG_COPY, SEG_COPY};
  ApplyTable t = {};
  long long blocks = 0;
  const float *const *src[3] = {params, exp_avgs, exp_avg_sqs};
  float *const *dst[3] = {out_params, out_exp_avgs, out_exp_avg_sqs};
  for (int g = 0; g < 3; ++g)
    for (int k = 0; k < 6; ++k) {
      if (width[k] == 0) continue;  // sh_bases 1: no features_rest, nothing launched for it
      if (!src[g][k] || !dst[g][k]) {
        set_error("density_apply: null tensor (set %d, parameter %d)", g, k);
        return 1;
      }
      ApplySeg &sg = t.seg[t.nseg];
      sg.src = src[g][k];
      sg.dst = dst[g][k];
      sg.width = width[k];
      sg.kind = g == 0 ? kind[k] : (k == 3 ? SEG_OPACITY_MOMENT : SEG_MOMENT);
      t.block0[t.nseg++] = blocks;
      blocks += ((long long)new_points * width[k] + DN_TPB * DN_VEC - 1) / (DN_TPB * DN_VEC);
    }
  t.block0[t.nseg] = blocks;
  if (blocks > 2147483647LL) {
    set_error("density_apply: too many blocks");
    return 1;
  }
  t.means = params[0];
  t.scales = params[1];
  t.quats = params[2];
  t.z = z;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(density_source_rows_kernel, dim3(cdiv(num_points, DN_TPB)), dim3(DN_TPB), 0,
                     st, num_points, new_points, n_split_samples, v.totals, v.flags, v.off_keep,
                     v.off_split, v.off_dup, src_rows);
  hipLaunchKernelGGL(density_gather_kernel, dim3((unsigned)blocks), dim3(DN_TPB), 0, st, t,
                     num_points, new_points, n_split_samples, v.totals, src_rows, reset_opacity,
                     opacity_cap);
  return check_launch("density_apply");
}
