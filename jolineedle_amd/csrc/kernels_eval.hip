// Detection evaluation on the device: merge_boxes (src/utils.py:198-255), and mAP-50 as compute_detection_metrics reports it
// (src/trainer.py:188-248; the COCO protocol of detection.map_50) split into a per-image matching and a per-segment
// average precision.  One workgroup per image / per segment throughout.
#include <hip/hip_runtime.h>

#include "jn_kernels.h"

// The IoU and the precision / recall arithmetic below must round exactly as the host's separate fp64 operations do: a fused
// multiply-add can flip a tie at IoU == 0.5.
#pragma clang fp contract(off)

namespace jnr {

constexpr int EV_NT = 256;

// Order-preserving image of an fp32 value in uint32 (negative values included), for integer atomic min / max.
__device__ __forceinline__ uint32_t ord_enc(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float ord_dec(uint32_t u) { return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

__device__ __forceinline__ bool boxes_adjacent(float ax1, float ay1, float ax2, float ay2, float bx1, float by1, float bx2,
                                               float by2, float thr) {
  const float d = fminf(fminf(fabsf(bx2 - ax1), fabsf(ax2 - bx1)), fminf(fabsf(by2 - ay1), fabsf(ay2 - by1)));
  return d <= thr;
}

// merge_boxes of one image per workgroup, in the parallel form of the reference's rule:
//   adj(i, j)  <=>  min(|b.x2 - a.x1|, |a.x2 - b.x1|, |b.y2 - a.y1|, |a.y2 - b.y1|) <= threshold     (fp32 subtractions)
//   r(j) = j where no i < j is adjacent to j, else the minimum of r(i) over those i        (the group that box j joins)
//   group g = {i : r(i) == g} and every j > i adjacent to such an i; groups in ascending g; output = min / max over members.
// Phase 1 relaxes r from r(j) = j in place until a workgroup-wide flag stays clear (the fixed point is unique, labels
// only fall, so reading a label another thread is lowering is harmless).  A label c on box i came down a chain of
// adjacent boxes c < ... < i, and r never rises along such a chain, so r(i) <= r(c) <= lab[c]: a box may take its
// label's label, which shortens a chain of n boxes from n - 1 rounds to about log n.  Phase 2 replaces, chunk by chunk in ascending
// order, the row of box i by the extent of {i} and its adjacent j > i — rows of a finished chunk are dead by then, later
// chunks only read higher rows.  Phase 3 folds the row of every non-root i into the row of its root r(i) with LDS
// atomics on the ordered-integer image; phase 4 compacts the roots (Hillis-Steele scan as in boxes_to_image_kernel).
// Dynamic LDS: [6][Nmax] words = x1, y1, x2, y2, obj * cls, label.
__global__ __launch_bounds__(EV_NT) void merge_boxes_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ counts,
                                                            int Nmax, int W, int off, float thr, float* __restrict__ out,
                                                            int32_t* __restrict__ out_counts, int32_t* __restrict__ out_rounds) {
  extern __shared__ uint32_t mb_sm[];
  __shared__ int32_t scan[2][EV_NT];
  __shared__ int32_t carry;
  __shared__ int32_t changed;
  float* x1 = (float*)mb_sm;
  float* y1 = x1 + Nmax;
  float* x2 = y1 + Nmax;
  float* y2 = x2 + Nmax;
  float* pr = y2 + Nmax;
  int32_t* lab = (int32_t*)(pr + Nmax);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(counts[b], 0), Nmax);
  const bool conf = (off == 0 && W > 5);
  const int Wout = off ? 5 : (conf ? 6 : 4);
  const float* src = boxes + (long long)b * Nmax * W;
  float* dst = out + (long long)b * Nmax * Wout;
  for (int i = tid; i < n; i += EV_NT) {
    const float* row = src + (long long)i * W;
    x1[i] = row[off + 0];
    y1[i] = row[off + 1];
    x2[i] = row[off + 2];
    y2[i] = row[off + 3];
    pr[i] = conf ? __fmul_rn(row[4], row[5]) : 0.0f;
    lab[i] = i;
  }
  // ---- phase 1: labels.  Box tid + k * EV_NT is bit k of `settled` once its label cannot fall any more (no lower
  // neighbour, or label 0); Nmax <= 4096 keeps k below 16.
  uint32_t settled = 0;
  int rounds = 0;
  for (;;) {
    __syncthreads();
    if (tid == 0) changed = 0;
    __syncthreads();
    bool ch = false;
    for (int j = tid, k = 0; j < n; j += EV_NT, ++k) {
      if ((settled >> k) & 1u) continue;
      const float ax1 = x1[j], ay1 = y1[j], ax2 = x2[j], ay2 = y2[j];
      const int cur = lab[j];
      int m = cur;
      bool any = false;
      for (int i = 0; i < j; ++i) {
        if (boxes_adjacent(x1[i], y1[i], x2[i], y2[i], ax1, ay1, ax2, ay2, thr)) {
          any = true;
          m = min(m, lab[i]);
          if (m == 0) break;
        }
      }
      while (lab[m] < m) m = lab[m];                         // r(j) <= r(m) <= lab[m]: follow the label's own label
      if (m < cur) {
        lab[j] = m;
        ch = true;
      }
      if (!any || m == 0) settled |= 1u << k;
    }
    if (ch) changed = 1;
    __syncthreads();
    ++rounds;
    if (!changed) break;
  }
  if (out_rounds && tid == 0) out_rounds[b] = rounds;
  // ---- phase 2: row i <- extent of {i} and its adjacent j > i, as ordered integers
  for (int i0 = 0; i0 < n; i0 += EV_NT) {
    const int i = i0 + tid;
    float mnx = 0.0f, mny = 0.0f, mxx = 0.0f, mxy = 0.0f, mp = 0.0f;
    if (i < n) {
      const float ax1 = x1[i], ay1 = y1[i], ax2 = x2[i], ay2 = y2[i];
      mnx = ax1, mny = ay1, mxx = ax2, mxy = ay2, mp = pr[i];
      for (int j = i + 1; j < n; ++j) {
        const float bx1 = x1[j], by1 = y1[j], bx2 = x2[j], by2 = y2[j];
        if (boxes_adjacent(ax1, ay1, ax2, ay2, bx1, by1, bx2, by2, thr)) {
          mnx = fminf(mnx, bx1);
          mny = fminf(mny, by1);
          mxx = fmaxf(mxx, bx2);
          mxy = fmaxf(mxy, by2);
          mp = fmaxf(mp, pr[j]);
        }
      }
    }
    __syncthreads();                                       // every read of this chunk's rows is done
    if (i < n) {
      mb_sm[i] = ord_enc(mnx);
      mb_sm[Nmax + i] = ord_enc(mny);
      mb_sm[2 * Nmax + i] = ord_enc(mxx);
      mb_sm[3 * Nmax + i] = ord_enc(mxy);
      mb_sm[4 * Nmax + i] = ord_enc(mp);
    }
  }
  __syncthreads();
  // ---- phase 3: fold every non-root row into its root's (a root is never read here, a non-root never written)
  for (int i = tid; i < n; i += EV_NT) {
    const int g = lab[i];
    if (g == i) continue;
    atomicMin(&mb_sm[g], mb_sm[i]);
    atomicMin(&mb_sm[Nmax + g], mb_sm[Nmax + i]);
    atomicMax(&mb_sm[2 * Nmax + g], mb_sm[2 * Nmax + i]);
    atomicMax(&mb_sm[3 * Nmax + g], mb_sm[3 * Nmax + i]);
    if (conf) atomicMax(&mb_sm[4 * Nmax + g], mb_sm[4 * Nmax + i]);
  }
  if (tid == 0) carry = 0;
  __syncthreads();
  // ---- phase 4: the roots, in ascending order, are the output rows
  for (int i0 = 0; i0 < n; i0 += EV_NT) {
    const int i = i0 + tid;
    const int c = (i < n && lab[i] == i) ? 1 : 0;
    int cur = 0;
    scan[0][tid] = c;
    __syncthreads();
    for (int d = 1; d < EV_NT; d <<= 1) {
      const int v = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0);
      scan[cur ^ 1][tid] = v;
      cur ^= 1;
      __syncthreads();
    }
    const int base = carry;
    if (c) {
      float* row = dst + (long long)(base + scan[cur][tid] - 1) * Wout;
      if (off) row[0] = 0.0f;
      row[off + 0] = ord_dec(mb_sm[i]);
      row[off + 1] = ord_dec(mb_sm[Nmax + i]);
      row[off + 2] = ord_dec(mb_sm[2 * Nmax + i]);
      row[off + 3] = ord_dec(mb_sm[3 * Nmax + i]);
      if (conf) {
        row[4] = ord_dec(mb_sm[4 * Nmax + i]);
        row[5] = 1.0f;
      }
    }
    __syncthreads();
    if (tid == EV_NT - 1) carry = base + scan[cur][tid];
    __syncthreads();
  }
  if (tid == 0) out_counts[b] = carry;
}

// Bitonic sort of np2 (a power of two) uint64 keys in LDS, ascending.
__device__ __forceinline__ void bitonic_sort_u64(unsigned long long* keys, int np2, int tid) {
  for (int k = 2; k <= np2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < np2; t += EV_NT) {
        const int u = t ^ j;
        if (u > t) {
          const unsigned long long a = keys[t], c = keys[u];
          if ((a > c) == ((t & k) == 0)) {
            keys[t] = c;
            keys[u] = a;
          }
        }
      }
      __syncthreads();
    }
  }
}

// The per-image half of detection.map_50.  Selection: the max_det best rows by column 4, descending, ties to the lower
// index (argsort(descending=True, stable=True)) — a bitonic sort of (inverted ordered score, index) keys.  Matching: the
// selected predictions in that order, each against the targets not yet taken: best starts at 0.5 and a target wins with
// iou >= best walking j upwards, i.e. the highest IoU and among equals the highest index.  IoU in fp64 in the host's
// operation order (_iou_matrix).  Dynamic LDS: uint64 [Npow2] keys.
__global__ __launch_bounds__(EV_NT) void match_detections_kernel(const float* __restrict__ preds, const int32_t* __restrict__ pcounts,
                                                                 int Nmax, int W, const float* __restrict__ tgts,
                                                                 const int32_t* __restrict__ tcounts, int Mmax, int max_det,
                                                                 double* __restrict__ scores, int32_t* __restrict__ hits,
                                                                 int32_t* __restrict__ sel, int32_t* __restrict__ n_pred,
                                                                 int32_t* __restrict__ n_gt) {
  extern __shared__ unsigned long long md_keys[];
  __shared__ uint32_t taken[JN_EVAL_MAX_BOXES / 32];
  __shared__ double wbest[EV_NT / 64];
  __shared__ int32_t wj[EV_NT / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(pcounts[b], 0), Nmax);
  const int m = Mmax > 0 ? min(max(tcounts[b], 0), Mmax) : 0;
  const float* src = preds + (long long)b * Nmax * W;
  const float* tg = tgts + (long long)b * Mmax * 5;
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = tid; i < np2; i += EV_NT)
    md_keys[i] = i < n ? ((unsigned long long)(~ord_enc(src[(long long)i * W + 4])) << 32) | (unsigned)i : ~0ull;
  for (int i = tid; i < JN_EVAL_MAX_BOXES / 32; i += EV_NT) taken[i] = 0;
  __syncthreads();
  bitonic_sort_u64(md_keys, np2, tid);
  const int ns = min(n, max_det);
  if (tid == 0) {
    n_pred[b] = ns;
    n_gt[b] = m;
  }
  for (int p = 0; p < ns; ++p) {
    const int idx = (int)(md_keys[p] & 0xFFFFFFFFull);
    const float* row = src + (long long)idx * W;
    const double a0 = row[0], a1 = row[1], a2 = row[2], a3 = row[3];
    const double area_a = (a2 - a0) * (a3 - a1);
    double best = 0.5;
    int bj = -1;
    for (int j = tid; j < m; j += EV_NT) {
      if ((taken[j >> 5] >> (j & 31)) & 1u) continue;
      const double b0 = tg[j * 5 + 1], b1 = tg[j * 5 + 2], b2 = tg[j * 5 + 3], b3 = tg[j * 5 + 4];
      const double w = fmax(fmin(a2, b2) - fmax(a0, b0), 0.0);
      const double h = fmax(fmin(a3, b3) - fmax(a1, b1), 0.0);
      const double inter = w * h;
      const double area_b = (b2 - b0) * (b3 - b1);
      const double iou = inter / fmax((area_a + area_b) - inter, 1e-12);
      if (iou >= best) {
        best = iou;
        bj = j;
      }
    }
    for (int d = 32; d > 0; d >>= 1) {
      const double ob = __shfl_xor(best, d);
      const int oj = __shfl_xor(bj, d);
      if (oj >= 0 && (bj < 0 || ob > best || (ob == best && oj > bj))) {
        best = ob;
        bj = oj;
      }
    }
    if ((tid & 63) == 0) {
      wbest[tid >> 6] = best;
      wj[tid >> 6] = bj;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < EV_NT / 64; ++w) {
        const double ob = wbest[w];
        const int oj = wj[w];
        if (oj >= 0 && (bj < 0 || ob > best || (ob == best && oj > bj))) {
          best = ob;
          bj = oj;
        }
      }
      if (bj >= 0) taken[bj >> 5] |= 1u << (bj & 31);
      const long long o = (long long)b * max_det + p;
      scores[o] = (double)row[4];
      hits[o] = bj >= 0 ? 1 : 0;
      sel[o] = idx;
    }
    __syncthreads();
  }
}

// Average precision of one segment of the concatenated (score, hit) lists per workgroup: a segment is `nimg` consecutive
// images (units) from img0, entry e of a segment is (image img0 + e / max_det, rank e % max_det), present where
// rank < n_pred.  Order by score descending, ties in concatenation order (Python's stable sorted); cumulative
// tp, precision = tp / (tp + fp), monotone envelope from the right; at every threshold the precision at the first
// index with recall >= threshold (0 past the end), summed sequentially in threshold order and divided by their number.
// Dynamic LDS: double [Npow2] (score, then precision envelope) + int32 [Npow2] (entry, then cumulative tp).  Shared by
// average_precision_kernel (one image or all of them) and average_precision_segments_kernel (a range of units).
__device__ __forceinline__ void average_precision_segment(const double* __restrict__ scores, const int32_t* __restrict__ hits,
                                                          const int32_t* __restrict__ n_pred, const int32_t* __restrict__ n_gt,
                                                          int img0, int nimg, int max_det, int Npow2,
                                                          const double* __restrict__ thresholds, int n_thr,
                                                          double* __restrict__ out) {
  extern __shared__ double ap_sm[];
  __shared__ int32_t iscan[2][EV_NT];
  __shared__ double dscan[2][EV_NT];
  __shared__ int32_t icarry, n_valid, gt_total;
  __shared__ double dcarry;
  __shared__ double terms[JN_EVAL_MAX_THRESHOLDS];
  double* val = ap_sm;
  int32_t* ent = (int32_t*)(ap_sm + Npow2);
  const int tid = threadIdx.x;
  const int slots = nimg * max_det;
  const long long base = (long long)img0 * max_det;
  if (tid == 0) n_valid = 0, gt_total = 0, icarry = 0;
  __syncthreads();
  int mine = 0, gts = 0;
  for (int e = tid; e < Npow2; e += EV_NT) {
    const bool valid = e < slots && (e % max_det) < n_pred[img0 + e / max_det];
    val[e] = valid ? scores[base + e] : -HUGE_VAL;
    ent[e] = e;
    mine += valid;
  }
  for (int i = tid; i < nimg; i += EV_NT) gts += n_gt[img0 + i];
  if (mine) atomicAdd(&n_valid, mine);
  if (gts) atomicAdd(&gt_total, gts);
  __syncthreads();
  const int n = n_valid, ngt = gt_total;
  if (n == 0 || ngt <= 0) {                               // map_50: no target / no prediction -> 0
    if (tid == 0) *out = 0.0;
    return;
  }
  for (int k = 2; k <= Npow2; k <<= 1) {                  // bitonic sort: (score descending, entry ascending)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < Npow2; t += EV_NT) {
        const int u = t ^ j;
        if (u > t) {
          const double va = val[t], vc = val[u];
          const int ea = ent[t], ec = ent[u];
          const bool after = va < vc || (va == vc && ea > ec);          // t's entry sorts after u's
          if (after == ((t & k) == 0)) {
            val[t] = vc, val[u] = va;
            ent[t] = ec, ent[u] = ea;
          }
        }
      }
      __syncthreads();
    }
  }
  // cumulative tp over the sorted order (chunks of EV_NT with a carry) -> ent[]; precision -> val[]
  for (int k0 = 0; k0 < n; k0 += EV_NT) {
    const int k = k0 + tid;
    const int c = (k < n && ent[k] < slots) ? (hits[base + ent[k]] != 0) : 0;   // (ent >= slots: only with non-finite scores)
    int cur = 0;
    iscan[0][tid] = c;
    __syncthreads();
    for (int d = 1; d < EV_NT; d <<= 1) {
      const int v = iscan[cur][tid] + (tid >= d ? iscan[cur][tid - d] : 0);
      iscan[cur ^ 1][tid] = v;
      cur ^= 1;
      __syncthreads();
    }
    const int tp = icarry + iscan[cur][tid];
    if (k < n) {
      ent[k] = tp;
      val[k] = (double)tp / (double)(k + 1);              // tp + fp == k + 1 exactly
    }
    __syncthreads();
    if (tid == EV_NT - 1) icarry = tp;
    __syncthreads();
  }
  // monotone envelope from the right: a running maximum over k = n - 1 .. 0
  if (tid == 0) dcarry = 0.0;
  __syncthreads();
  for (int q0 = 0; q0 < n; q0 += EV_NT) {
    const int q = q0 + tid, k = n - 1 - q;
    const double c = q < n ? val[k] : 0.0;
    int cur = 0;
    dscan[0][tid] = c;
    __syncthreads();
    for (int d = 1; d < EV_NT; d <<= 1) {
      const double v = tid >= d ? fmax(dscan[cur][tid], dscan[cur][tid - d]) : dscan[cur][tid];
      dscan[cur ^ 1][tid] = v;
      cur ^= 1;
      __syncthreads();
    }
    const double env = fmax(dcarry, dscan[cur][tid]);
    if (q < n) val[k] = env;
    __syncthreads();
    if (tid == EV_NT - 1) dcarry = env;
    __syncthreads();
  }
  for (int t = tid; t < n_thr; t += EV_NT) {
    const double r = thresholds[t];
    int lo = 0, hi = n;                                   // searchsorted(recall, r, right=False)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((double)ent[mid] / (double)ngt >= r) hi = mid; else lo = mid + 1;
    }
    terms[t] = lo < n ? val[lo] : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    double ap = 0.0;
    for (int t = 0; t < n_thr; ++t) ap += terms[t];
    *out = ap / (double)n_thr;
  }
}

// segment s is image s (pooled = 0) or all B images (pooled = 1)
__global__ __launch_bounds__(EV_NT) void average_precision_kernel(const double* __restrict__ scores, const int32_t* __restrict__ hits,
                                                                  const int32_t* __restrict__ n_pred,
                                                                  const int32_t* __restrict__ n_gt, int B, int max_det,
                                                                  int pooled, int Npow2, const double* __restrict__ thresholds,
                                                                  int n_thr, double* __restrict__ out) {
  average_precision_segment(scores, hits, n_pred, n_gt, pooled ? 0 : (int)blockIdx.x, pooled ? B : 1, max_det, Npow2, thresholds,
                            n_thr, out + blockIdx.x);
}

// segment s is the units seg_offsets[s] .. seg_offsets[s + 1] - 1 (kept inside 0..U and at most max_units long: the LDS
// was sized for that many)
__global__ __launch_bounds__(EV_NT) void average_precision_segments_kernel(const double* __restrict__ scores,
                                                                           const int32_t* __restrict__ hits,
                                                                           const int32_t* __restrict__ n_pred,
                                                                           const int32_t* __restrict__ n_gt, int U, int max_det,
                                                                           const int32_t* __restrict__ seg_offsets, int max_units,
                                                                           int Npow2, const double* __restrict__ thresholds,
                                                                           int n_thr, double* __restrict__ out) {
  const int u0 = min(max(seg_offsets[blockIdx.x], 0), U);
  const int u1 = min(max(seg_offsets[blockIdx.x + 1], u0), U);
  average_precision_segment(scores, hits, n_pred, n_gt, u0, min(u1 - u0, max_units), max_det, Npow2, thresholds, n_thr,
                            out + blockIdx.x);
}

// Inclusive sum of one int per thread over the workgroup (Hillis-Steele in LDS, as the compactions above); every thread
// calls it, and the buffer is free again when it returns.
__device__ __forceinline__ int block_scan_inclusive(int v, int32_t (*scan)[EV_NT], int tid) {
  int cur = 0;
  scan[0][tid] = v;
  __syncthreads();
  for (int d = 1; d < EV_NT; d <<= 1) {
    const int s = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0);
    scan[cur ^ 1][tid] = s;
    cur ^= 1;
    __syncthreads();
  }
  const int r = scan[cur][tid];
  __syncthreads();
  return r;
}

// The multistart evaluation's pool + NMS (src/supervised.py:573-625) for one (cell, image) per workgroup: the boxes of
// every token of the image's used walks that stands on the cell, in (walk, token, stored) order, de-duplicated greedily
// in (score descending, pool index ascending) order at IoU > 0.5 in fp32.  A token slot of the image is
// e = walk * (S + 1) + t, a box slot r = e * K + k < cap <= JN_EVAL_MAX_BOXES, so both the pool index and r fit 16 bits
// of the sort key: key = (inverted ordered score) << 32 | pool << 16 | r.  Dynamic LDS: uint64 [cap2] keys, then
// float [4][cap] x1, y1, x2, y2 at the POOL index (24 B per box where cap is a power of two).
__global__ __launch_bounds__(EV_NT) void pool_walk_detections_kernel(
    const float* __restrict__ det_boxes, const int32_t* __restrict__ det_counts, const int64_t* __restrict__ positions,
    const int32_t* __restrict__ walk_tokens, const int32_t* __restrict__ walk_first, const int32_t* __restrict__ walk_count,
    int A, int T, int S, int K, int max_walks, int Gw, int M, int cap, int cap2, float* __restrict__ cell_boxes,
    int32_t* __restrict__ cell_counts, int32_t* __restrict__ cell_stats, uint8_t* __restrict__ visited) {
  extern __shared__ unsigned long long pw_keys[];
  __shared__ int32_t scan[2][EV_NT];
  __shared__ uint32_t dead[JN_EVAL_MAX_BOXES / 32];
  __shared__ int32_t carry, seen;
  float* x1 = (float*)(pw_keys + cap2);
  float* y1 = x1 + cap;
  float* x2 = y1 + cap;
  float* y2 = x2 + cap;
  const int tid = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
  const int cells = gridDim.x;
  const long long cy = c / Gw, cx = c % Gw;
  const int w0 = walk_first[img];
  const int nw = min(max(walk_count[img], 0), max_walks);
  const int slots = nw * (S + 1);
  const long long unit = (long long)img * cells + c;
  if (tid == 0) carry = 0, seen = 0;
  for (int i = tid; i < JN_EVAL_MAX_BOXES / 32; i += EV_NT) dead[i] = 0;
  __syncthreads();
  // ---- the tokens on this cell and their boxes: pool offsets by a scan over the token slots
  for (int e0 = 0; e0 < slots; e0 += EV_NT) {
    const int e = e0 + tid;
    int cnt = 0;
    long long tok = 0;
    if (e < slots) {
      const int a = w0 + e / (S + 1), t = e % (S + 1);
      if (a >= 0 && a < A && t < walk_tokens[a]) {
        tok = (long long)a * (T + 1) + t;
        if (positions[tok * 2] == cy && positions[tok * 2 + 1] == cx) {
          seen = 1;
          cnt = min(max(det_counts[tok], 0), K);
        }
      }
    }
    const int before = carry;                              // stable since the barrier that ended the last chunk
    const int incl = block_scan_inclusive(cnt, scan, tid);
    const int base = before + incl - cnt;
    for (int k = 0; k < cnt; ++k) {
      const float* row = det_boxes + (tok * K + k) * 7;
      const int p = base + k;
      x1[p] = row[0], y1[p] = row[1], x2[p] = row[2], y2[p] = row[3];
      // ord_enc orders bit patterns: -0.0 ranks below +0.0 and a NaN by its bits, where the host's stable argsort holds
      // +-0 equal and puts NaN first.  Scores are sigmoid products in (0, 1], so neither occurs (as in match_detections).
      pw_keys[p] = ((unsigned long long)(~ord_enc(row[4])) << 32) | ((unsigned)p << 16) | (unsigned)(e * K + k);
    }
    if (tid == EV_NT - 1) carry = before + incl;
    __syncthreads();
  }
  const int n = carry;
  if (n == 0) {                                            // an unvisited cell, or a visited one whose tokens hold no box
    if (tid == 0) {
      cell_counts[unit] = 0;
      visited[unit] = seen ? 1 : 0;
      if (cell_stats) cell_stats[unit * 2] = 0, cell_stats[unit * 2 + 1] = 0;
    }
    return;
  }
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = n + tid; i < np2; i += EV_NT) pw_keys[i] = ~0ull;
  __syncthreads();
  bitonic_sort_u64(pw_keys, np2, tid);
  // ---- greedy NMS: the kept box of rank p against every later live box, one round per kept box
  for (int p = 0; p + 1 < n; ++p) {
    if ((dead[p >> 5] >> (p & 31)) & 1u) continue;          // uniform: written before the last barrier
    const int pi = (int)((pw_keys[p] >> 16) & 0xFFFFu);
    const float ax1 = x1[pi], ay1 = y1[pi], ax2 = x2[pi], ay2 = y2[pi];
    const float area_a = (ax2 - ax1) * (ay2 - ay1);
    for (int q = p + 1 + tid; q < n; q += EV_NT) {
      if ((dead[q >> 5] >> (q & 31)) & 1u) continue;
      const int qi = (int)((pw_keys[q] >> 16) & 0xFFFFu);
      const float bx1 = x1[qi], by1 = y1[qi], bx2 = x2[qi], by2 = y2[qi];
      const float w = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.0f);
      const float h = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.0f);
      const float inter = w * h;
      const float area_b = (bx2 - bx1) * (by2 - by1);
      const float iou = __fdiv_rn(inter, (area_a + area_b) - inter);
      if (iou > 0.5f) atomicOr(&dead[q >> 5], 1u << (q & 31));      // (a NaN compares false)
    }
    __syncthreads();
  }
  // ---- the survivors in score order: rows 0 .. min(survivors, M) - 1
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int p0 = 0; p0 < n; p0 += EV_NT) {
    const int p = p0 + tid;
    const int live = (p < n && !((dead[p >> 5] >> (p & 31)) & 1u)) ? 1 : 0;
    const int before = carry;
    const int incl = block_scan_inclusive(live, scan, tid);
    const int rank = before + incl - 1;
    if (live && rank < M) {
      const int r = (int)(pw_keys[p] & 0xFFFFu);
      const int e = r / K, k = r % K;
      const long long tok = (long long)(w0 + e / (S + 1)) * (T + 1) + e % (S + 1);
      const float* row = det_boxes + (tok * K + k) * 7;
      float* dst = cell_boxes + (unit * M + rank) * 7;
      for (int j = 0; j < 7; ++j) dst[j] = row[j];
    }
    if (tid == EV_NT - 1) carry = before + incl;
    __syncthreads();
  }
  if (tid == 0) {
    cell_counts[unit] = min(carry, M);
    visited[unit] = 1;
    if (cell_stats) cell_stats[unit * 2] = n, cell_stats[unit * 2 + 1] = carry;
  }
}

int launch_merge_boxes(const float* boxes, const int32_t* counts, int B, int Nmax, int W, int target, float threshold,
                       float* out_boxes, int32_t* out_counts, int32_t* out_rounds, hipStream_t s) {
  const size_t smem = (size_t)6 * Nmax * sizeof(uint32_t);
  if (!allow_lds<&merge_boxes_kernel>(smem)) return 1;
  hipLaunchKernelGGL(merge_boxes_kernel, dim3(B), dim3(EV_NT), smem, s, boxes, counts, Nmax, W, target ? 1 : 0, threshold,
                     out_boxes, out_counts, out_rounds);
  return 0;
}

int launch_match_detections(const float* preds, const int32_t* pred_counts, int B, int Nmax, int W, const float* targets,
                            const int32_t* target_counts, int Mmax, int max_det, double* scores, int32_t* hits, int32_t* sel,
                            int32_t* n_pred, int32_t* n_gt, hipStream_t s) {
  int np2 = 1;
  while (np2 < Nmax) np2 <<= 1;
  const size_t smem = (size_t)np2 * sizeof(unsigned long long);
  hipLaunchKernelGGL(match_detections_kernel, dim3(B), dim3(EV_NT), smem, s, preds, pred_counts, Nmax, W, targets, target_counts,
                     Mmax, max_det, scores, hits, sel, n_pred, n_gt);
  return 0;
}

int launch_average_precision(const double* scores, const int32_t* hits, const int32_t* n_pred, const int32_t* n_gt, int B,
                             int max_det, int pooled, const double* thresholds, int n_thresholds, double* out, hipStream_t s) {
  const int slots = (pooled ? B : 1) * max_det;
  int np2 = 2;
  while (np2 < slots) np2 <<= 1;
  const size_t smem = (size_t)np2 * (sizeof(double) + sizeof(int32_t));
  if (!allow_lds<&average_precision_kernel>(smem)) return 1;
  hipLaunchKernelGGL(average_precision_kernel, dim3(pooled ? 1 : B), dim3(EV_NT), smem, s, scores, hits, n_pred, n_gt, B, max_det,
                     pooled, np2, thresholds, n_thresholds, out);
  return 0;
}

int launch_pool_walk_detections(const float* det_boxes, const int32_t* det_counts, const int64_t* positions,
                                const int32_t* walk_tokens, const int32_t* walk_first, const int32_t* walk_count, int A, int T,
                                int S, int K, int NI, int max_walks, int Gh, int Gw, int M, float* cell_boxes,
                                int32_t* cell_counts, int32_t* cell_stats, uint8_t* visited, hipStream_t s) {
  const int cap = max_walks * (S + 1) * K;
  int cap2 = 1;
  while (cap2 < cap) cap2 <<= 1;
  const size_t smem = (size_t)cap2 * sizeof(unsigned long long) + (size_t)4 * cap * sizeof(float);
  if (!allow_lds<&pool_walk_detections_kernel>(smem)) return 1;
  hipLaunchKernelGGL(pool_walk_detections_kernel, dim3(Gh * Gw, NI), dim3(EV_NT), smem, s, det_boxes, det_counts, positions,
                     walk_tokens, walk_first, walk_count, A, T, S, K, max_walks, Gw, M, cap, cap2, cell_boxes, cell_counts,
                     cell_stats, visited);
  return 0;
}

int launch_average_precision_segments(const double* scores, const int32_t* hits, const int32_t* n_pred, const int32_t* n_gt,
                                      int U, int max_det, const int32_t* seg_offsets, int NS, int max_units,
                                      const double* thresholds, int n_thresholds, double* out, hipStream_t s) {
  const int slots = max_units * max_det;
  int np2 = 2;
  while (np2 < slots) np2 <<= 1;
  const size_t smem = (size_t)np2 * (sizeof(double) + sizeof(int32_t));
  if (!allow_lds<&average_precision_segments_kernel>(smem)) return 1;
  hipLaunchKernelGGL(average_precision_segments_kernel, dim3(NS), dim3(EV_NT), smem, s, scores, hits, n_pred, n_gt, U, max_det,
                     seg_offsets, max_units, np2, thresholds, n_thresholds, out);
  return 0;
}

}  // namespace jnr
