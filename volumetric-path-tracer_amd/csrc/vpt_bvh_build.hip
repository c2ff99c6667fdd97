// vpt_bvh_build.hip — the reference's BVH build on the device: build_bvh(bvh, bboxes, highquality)
// (libs/yocto/yocto_bvh.cpp:447-507) with split_middle (:411-441) or split_sah (:317-373, below), reproduced NODE FOR NODE: same node array (ids in the
// reference's creation order), same primitive order, same float bits.  SURVEY §8(f) row 4; include/vpt.h: vpt_build_bvh.
//
// The reference builds depth first from an explicit stack; a node's ids and its primitives' order are by-products of that
// order and of libstdc++'s std::partition.  Here the tree grows one LEVEL per round over all of the level's nodes at
// once, and three observations make the result identical:
//
//  * bounds.  merge() folds min(a, b) = a < b ? a : b and max(a, b) = a > b ? a : b over the node's primitives in array
//    order, so among equal candidates the LAST one wins - visible only as the sign of a zero.  A parallel reduction over
//    the key (value with -0 == +0, position in the primitive array) with the later position preferred picks the same
//    element; the result's bits are then read from that element.  Keys are 64-bit: atomicMin / atomicMax.
//  * partition.  libstdc++'s std::partition (bidirectional form, stl_algo.h __partition) walks inwards from both ends and
//    swaps the k-th element from the left that fails the predicate with the k-th from the right that passes it, while
//    the former is left of the latter.  If the range holds T passing elements, these are exactly the failing elements at
//    positions < start + T and the passing ones at positions >= start + T, paired in that order; nothing else moves.
//    With an exclusive scan of the predicate over the whole primitive array every element finds its rank, hence its
//    partner, on its own.
//  * node ids.  The reference appends a node's two children when the node is popped, and pops the right child first: ids
//    follow the pre-order that visits right subtrees first.  With icount(X) = internal nodes in X's subtree and
//    pre(X) = internal nodes visited before X: pre(right) = pre(P) + 1, pre(left) = pre(P) + 1 + icount(right), and the
//    children of X sit at 1 + 2 pre(X), 2 + 2 pre(X).  Two sweeps over the levels (up for icount, down for pre).
//
// Two parts: bvh_build_core (vpt_bvh_build.h) takes boxes that are on the device and leaves nodes and primitive order there -
// vpt_scene_rebuild_bvh (vpt_bvh_rebuild.hip) runs it on boxes made from a resident scene - and vpt_build_bvh wraps it with the
// copies from and to the host.
// Work per level: O(n) threads, a handful of 64-bit atomics per live primitive, one rocPRIM scan.  The host reads back
// one counter per level (the number of nodes the level created).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "vpt_bvh_build.h"
#include "vpt_device_buffer.h"
#include "vpt_error.h"

namespace {

constexpr int BVH_MAX_PRIMS = 4;   // yocto_bvh.cpp:444

// a node under construction, in creation (level) order
struct tnode {
  int start, end;      // its range of the primitive array
  int parent, which;   // temp id of the parent (-1: root), 0 = left / 1 = right child
  int child;           // temp id of the left child (right = child + 1), -1: leaf
  int axis, mid, swap; // split_middle's result; swap: the partition moves elements
  float split;
  int icount, pre;     // internal nodes in the subtree / visited before this node in the reference's order
};
struct tkeys {   // reduction keys: [0..2] min of bbox.min, [3..5] max of bbox.max, [6..8] min of centres, [9..11] max of centres
  unsigned long long k[12];
};

__device__ __forceinline__ unsigned ordered(float f) {   // monotone float -> unsigned, -0 and +0 alike
  unsigned u = __float_as_uint(f == 0.0f ? 0.0f : f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long min_key(float f, int pos) { return (unsigned long long)ordered(f) << 32 | (0xffffffffu - (unsigned)pos); }
__device__ __forceinline__ unsigned long long max_key(float f, int pos) { return (unsigned long long)ordered(f) << 32 | (unsigned)pos; }
__device__ __forceinline__ int min_pos(unsigned long long k) { return (int)(0xffffffffu - (unsigned)(k & 0xffffffffull)); }
__device__ __forceinline__ int max_pos(unsigned long long k) { return (int)(k & 0xffffffffull); }

// (bb: box p = the six floats at bb + stride * p)
__global__ void k_centers(int n, const float* __restrict__ bb, int stride, float* __restrict__ ctr) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int c = 0; c < 3; c++) ctr[3 * i + c] = (bb[(size_t)stride * i + c] + bb[(size_t)stride * i + 3 + c]) / 2;   // center(bbox), yocto_geometry.h: (min + max) / 2
}
__global__ void k_init(int n, int* prims, int* node_of) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) prims[i] = i, node_of[i] = 0;
}
__global__ void k_reset_keys(int lb, int le, tkeys* keys) {
  int t = lb + blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= le) return;
  for (int c = 0; c < 3; c++) keys[t].k[c] = keys[t].k[6 + c] = ~0ull, keys[t].k[3 + c] = keys[t].k[9 + c] = 0ull;
}
// bounds of every live node: each primitive position offers its box and its centre to its node.  Positions of a node are
// contiguous, so near the root all 64 lanes of a wave belong to the same node: they fold their keys across the wave first and
// lane 0 makes the 12 atomic updates (without this the first levels serialise n atomics on 12 addresses).
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
  for (int m = 32; m >= 1; m >>= 1) {
    unsigned long long o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int m = 32; m >= 1; m >>= 1) {
    unsigned long long o = __shfl_xor(v, m, 64);
    v = o > v ? o : v;
  }
  return v;
}
__global__ void k_bounds(int n, const int* __restrict__ prims, const int* __restrict__ node_of, const float* __restrict__ bb, int stride,
    const float* __restrict__ ctr, tkeys* keys) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int t = i < n ? node_of[i] : -1;
  int t0 = __builtin_amdgcn_readfirstlane(t);
  bool uniform = __builtin_amdgcn_ballot_w64(t != t0) == 0;   // the whole wave (blockDim is a multiple of 64) in one node
  if (uniform && t0 < 0) return;
  unsigned long long k[12];
  if (t >= 0) {
    int p = prims[i];
    for (int c = 0; c < 3; c++) {
      k[c]     = min_key(bb[(size_t)stride * p + c], i);
      k[3 + c] = max_key(bb[(size_t)stride * p + 3 + c], i);
      k[6 + c] = min_key(ctr[3 * p + c], i);
      k[9 + c] = max_key(ctr[3 * p + c], i);
    }
  }
  if (uniform) {
    for (int c = 0; c < 3; c++) k[c] = wave_min(k[c]), k[3 + c] = wave_max(k[3 + c]), k[6 + c] = wave_min(k[6 + c]), k[9 + c] = wave_max(k[9 + c]);
    if ((threadIdx.x & 63) != 0) return;
  } else if (t < 0) return;
  for (int c = 0; c < 3; c++) {
    atomicMin(&keys[t].k[c], k[c]);
    atomicMax(&keys[t].k[3 + c], k[3 + c]);
    atomicMin(&keys[t].k[6 + c], k[6 + c]);
    atomicMax(&keys[t].k[9 + c], k[9 + c]);
  }
}
// the node's box (bits of the winning elements) and split_middle's choice of axis and plane
__global__ void k_decide(int lb, int le, tnode* nodes, const tkeys* keys, const int* __restrict__ prims, const float* __restrict__ bb, int stride,
    const float* __restrict__ ctr, float* boxes) {
  int t = lb + blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= le) return;
  tnode& nd = nodes[t];
  for (int c = 0; c < 3; c++) {
    boxes[6 * t + c]     = bb[(size_t)stride * prims[min_pos(keys[t].k[c])] + c];
    boxes[6 * t + 3 + c] = bb[(size_t)stride * prims[max_pos(keys[t].k[3 + c])] + 3 + c];
  }
  nd.child = -1, nd.axis = 0, nd.swap = 0, nd.mid = (nd.start + nd.end) / 2, nd.split = 0;
  if (nd.end - nd.start <= BVH_MAX_PRIMS) return;   // a leaf
  float cmin[3], cmax[3], csize[3];
  for (int c = 0; c < 3; c++) {
    cmin[c]  = ctr[3 * prims[min_pos(keys[t].k[6 + c])] + c];
    cmax[c]  = ctr[3 * prims[max_pos(keys[t].k[9 + c])] + c];
    csize[c] = cmax[c] - cmin[c];
  }
  nd.child = -2;   // internal; the children are allocated by k_children
  if (csize[0] == 0 && csize[1] == 0 && csize[2] == 0) return;   // :422: halves, axis 0
  int axis = 0;
  if (csize[0] >= csize[1] && csize[0] >= csize[2]) axis = 0;
  if (csize[1] >= csize[0] && csize[1] >= csize[2]) axis = 1;
  if (csize[2] >= csize[0] && csize[2] >= csize[1]) axis = 2;
  nd.axis = axis, nd.split = (cmin[axis] + cmax[axis]) / 2, nd.swap = 1;
}
// ---- split_sah (include/vpt.h: vpt_build_bvh_quality) --------------------------------------------------------------------
// A node of more than four primitives whose centre box has a size searches 45 planes: 15 borders on each axis.  The borders of an axis
// do not decrease with b, so the 15 left sets are nested: a primitive's bin is the number of borders its centre is NOT below, and the
// left side of candidate b is bins 0 .. b-1.  A bin holds a count and a box; counts add and boxes merge with integer atomics (min / max
// on the ordered() image of the floats), which do not depend on order - the image forgets only the sign of a zero, and area() adds that
// to 1e-12f.  A node whose borders do decrease (a NaN csize) is searched candidate by candidate, in array order, as the reference does.
// The ranges of a level's nodes are disjoint, so start / 5 names a slot of its own for every node of five primitives or more.
constexpr int      SAH_BINS = 16, SAH_WORDS = 7;                  // per bin: the count, min.xyz and max.xyz as ordered() images
constexpr int      SAH_SLOT_WORDS = 3 * SAH_BINS * SAH_WORDS;     // 336 words = 1344 B per node
constexpr unsigned SAH_EMPTY_MIN = 0xff7fffffu, SAH_EMPTY_MAX = 0x00800000u;   // ordered(flt_max), ordered(-flt_max): the invalid box
constexpr float    SAH_FLT_MAX = 3.402823466e+38f;
struct sah_node_info {   // of a slot: the centre box of its node and how it is searched
  float cmin[3], csize[3];
  int   direct;     // the borders of an axis decrease somewhere: no bins, k_decide_sah walks the primitives
  int   pad;
};
__device__ __forceinline__ float unordered(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ unsigned sah_empty_word(int w) { return w == 0 ? 0u : (w <= 3 ? SAH_EMPTY_MIN : SAH_EMPTY_MAX); }
__device__ __forceinline__ float sah_border(float cmin, float csize, int b) { return cmin + ((float)b * csize) / 16.0f; }
__device__ __forceinline__ float sah_area(float sx, float sy, float sz) { return ((1e-12f + (2 * sx) * sy) + (2 * sx) * sz) + (2 * sy) * sz; }

__global__ void k_sah_clear(size_t words, unsigned* bins) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < words) bins[j] = sah_empty_word((int)(j % SAH_WORDS));
}
// per node of the level: its slot (-1: a leaf, or all centres alike - nothing to search), centre box and search form
__global__ void k_sah_prepare(int lb, int le, const tnode* __restrict__ nodes, const tkeys* __restrict__ keys, const int* __restrict__ prims,
    const float* __restrict__ ctr, int* __restrict__ sah_slot, sah_node_info* __restrict__ info) {
  int t = lb + blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= le) return;
  const tnode& nd = nodes[t];
  sah_slot[t] = -1;
  if (nd.end - nd.start <= BVH_MAX_PRIMS) return;
  sah_node_info f;
  for (int c = 0; c < 3; c++) {
    f.cmin[c]  = ctr[3 * prims[min_pos(keys[t].k[6 + c])] + c];
    f.csize[c] = ctr[3 * prims[max_pos(keys[t].k[9 + c])] + c] - f.cmin[c];
  }
  if (f.csize[0] == 0 && f.csize[1] == 0 && f.csize[2] == 0) return;
  f.direct = 0, f.pad = 0;
  for (int c = 0; c < 3; c++)
    for (int b = 1; b < SAH_BINS - 1; b++)
      if (!(sah_border(f.cmin[c], f.csize[c], b) <= sah_border(f.cmin[c], f.csize[c], b + 1))) f.direct = 1;
  const int slot = nd.start / (BVH_MAX_PRIMS + 1);
  info[slot] = f, sah_slot[t] = slot;
}
// every primitive position offers its count and box to one bin per axis of its node.  A block whose positions all belong to one node
// (every block but two of a node near the root) folds them in LDS first and sends each bin it touched once.
__global__ void __launch_bounds__(256) k_sah_bin(int n, const int* __restrict__ prims, const int* __restrict__ node_of, const int* __restrict__ sah_slot,
    const sah_node_info* __restrict__ info, const float* __restrict__ bb, int stride, const float* __restrict__ ctr, unsigned* bins) {
  __shared__ unsigned sb[SAH_SLOT_WORDS];
  __shared__ int      s_t0;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int t = i < n ? node_of[i] : -1;
  if (threadIdx.x == 0) s_t0 = t;
  __syncthreads();
  const int  t0 = s_t0;
  const bool uniform = __syncthreads_and(t == t0) != 0;
  int        slot = t >= 0 ? sah_slot[t] : -1;
  if (slot >= 0 && info[slot].direct) slot = -1;
  if (uniform && slot < 0) return;   // the whole block: nothing to bin
  unsigned* dst = uniform ? sb : bins + (size_t)(slot < 0 ? 0 : slot) * SAH_SLOT_WORDS;
  if (uniform) {
    for (int j = threadIdx.x; j < SAH_SLOT_WORDS; j += blockDim.x) sb[j] = sah_empty_word(j % SAH_WORDS);
    __syncthreads();
  }
  if (slot >= 0) {
    const sah_node_info& f = info[slot];
    const int       p = prims[i];
    unsigned        lo[3], hi[3];
    for (int c = 0; c < 3; c++) lo[c] = ordered(bb[(size_t)stride * p + c]), hi[c] = ordered(bb[(size_t)stride * p + 3 + c]);
    for (int a = 0; a < 3; a++) {
      const float x = ctr[3 * p + a];
      int         bin = 0;
      for (int b = 1; b < SAH_BINS; b++) bin += (x < sah_border(f.cmin[a], f.csize[a], b)) ? 0 : 1;
      unsigned* w = dst + (a * SAH_BINS + bin) * SAH_WORDS;
      atomicAdd(&w[0], 1u);
      for (int c = 0; c < 3; c++) atomicMin(&w[1 + c], lo[c]), atomicMax(&w[4 + c], hi[c]);
    }
  }
  if (!uniform) return;
  __syncthreads();
  unsigned* out = bins + (size_t)slot * SAH_SLOT_WORDS;   // (uniform: every thread holds the block's slot)
  for (int j = threadIdx.x; j < SAH_SLOT_WORDS; j += blockDim.x) {
    const int      w = j % SAH_WORDS;
    const unsigned v = sb[j];
    if (v == sah_empty_word(w)) continue;
    if (w == 0) atomicAdd(&out[j], v);
    else if (w <= 3) atomicMin(&out[j], v);
    else atomicMax(&out[j], v);
  }
}
// k_decide with split_sah's choice of axis and plane: one wave per node of the level, lane 16 saxis + b costs candidate (saxis, b)
__global__ void __launch_bounds__(64) k_decide_sah(int lb, int le, tnode* nodes, const tkeys* keys, const int* __restrict__ prims, const float* __restrict__ bb,
    int stride, const float* __restrict__ ctr, float* boxes, const int* __restrict__ sah_slot, const sah_node_info* __restrict__ info, unsigned* bins) {
  const int t = lb + blockIdx.x, lane = threadIdx.x;   // (the grid has le - lb blocks)
  tnode&    nd = nodes[t];
  const int start = nd.start, end = nd.end, slot = sah_slot[t];
  if (lane < 3) boxes[6 * t + lane] = bb[(size_t)stride * prims[min_pos(keys[t].k[lane])] + lane];
  else if (lane < 6) boxes[6 * t + lane] = bb[(size_t)stride * prims[max_pos(keys[t].k[lane])] + lane];
  if (lane == 0) nd.child = end - start <= BVH_MAX_PRIMS ? -1 : -2, nd.axis = 0, nd.swap = 0, nd.mid = (start + end) / 2, nd.split = 0;
  if (slot < 0) return;   // a leaf, or halves on axis 0; the same for the whole wave
  const sah_node_info f = info[slot];
  const int      saxis = lane >> 4, b = lane & 15;
  const bool     candidate = saxis < 3 && b >= 1;
  const int      a = candidate ? saxis : 0;
  const float    bsplit = sah_border(f.cmin[a], f.csize[a], b);
  float          lmin[3], lmax[3], rmin[3], rmax[3];
  int            ln = 0, rn = 0;
  if (!f.direct) {
    unsigned        ulo[3] = {SAH_EMPTY_MIN, SAH_EMPTY_MIN, SAH_EMPTY_MIN}, uhi[3] = {SAH_EMPTY_MAX, SAH_EMPTY_MAX, SAH_EMPTY_MAX};
    unsigned        vlo[3] = {SAH_EMPTY_MIN, SAH_EMPTY_MIN, SAH_EMPTY_MIN}, vhi[3] = {SAH_EMPTY_MAX, SAH_EMPTY_MAX, SAH_EMPTY_MAX};
    const unsigned* w = bins + (size_t)slot * SAH_SLOT_WORDS + (size_t)a * SAH_BINS * SAH_WORDS;
    for (int k = 0; k < SAH_BINS; k++, w += SAH_WORDS) {
      if (k < b) {
        ln += (int)w[0];
        for (int c = 0; c < 3; c++) ulo[c] = min(ulo[c], w[1 + c]), uhi[c] = max(uhi[c], w[4 + c]);
      } else {
        rn += (int)w[0];
        for (int c = 0; c < 3; c++) vlo[c] = min(vlo[c], w[1 + c]), vhi[c] = max(vhi[c], w[4 + c]);
      }
    }
    for (int c = 0; c < 3; c++) lmin[c] = unordered(ulo[c]), lmax[c] = unordered(uhi[c]), rmin[c] = unordered(vlo[c]), rmax[c] = unordered(vhi[c]);
  } else {
    for (int c = 0; c < 3; c++) lmin[c] = rmin[c] = SAH_FLT_MAX, lmax[c] = rmax[c] = -SAH_FLT_MAX;
    for (int i = start; i < end && candidate; i++) {   // merge(), yocto_math.h: min(a, b) = a < b ? a : b over the primitives in array order
      const int p = prims[i];
      if (ctr[3 * p + a] < bsplit) {
        ln++;
        for (int c = 0; c < 3; c++) {
          const float x = bb[(size_t)stride * p + c], y = bb[(size_t)stride * p + 3 + c];
          lmin[c] = lmin[c] < x ? lmin[c] : x, lmax[c] = lmax[c] > y ? lmax[c] : y;
        }
      } else {
        rn++;
        for (int c = 0; c < 3; c++) {
          const float x = bb[(size_t)stride * p + c], y = bb[(size_t)stride * p + 3 + c];
          rmin[c] = rmin[c] < x ? rmin[c] : x, rmax[c] = rmax[c] > y ? rmax[c] : y;
        }
      }
    }
  }
  const float carea = sah_area(f.csize[0], f.csize[1], f.csize[2]);   // of the CENTRE box, as the reference has it
  const float larea = sah_area(lmax[0] - lmin[0], lmax[1] - lmin[1], lmax[2] - lmin[2]);
  const float rarea = sah_area(rmax[0] - rmin[0], rmax[1] - rmin[1], rmax[2] - rmin[2]);
  const float cost = (1 + ((float)ln * larea) / carea) + ((float)rn * rarea) / carea;
  // the reference takes a candidate when cost < min_cost, from flt_max, in lane order: the first lane that holds the least cost below flt_max
  unsigned long long key = (candidate && cost < SAH_FLT_MAX) ? ((unsigned long long)ordered(cost) << 32 | (unsigned)lane) : ~0ull;
  key = wave_min(key);
  const int   winner = key == ~0ull ? 0 : (int)(key & 63ull);
  const float split = __shfl(bsplit, winner, 64);
  if (lane == 0) nd.axis = key == ~0ull ? 0 : winner >> 4, nd.split = key == ~0ull ? 0.0f : split, nd.swap = 1;
  __syncthreads();   // every lane has read the bins: leave them empty for the node that takes this slot on the next level
  if (!f.direct && lane < 3 * SAH_BINS) {
    unsigned* w = bins + (size_t)slot * SAH_SLOT_WORDS + (size_t)lane * SAH_WORDS;
    for (int c = 0; c < SAH_WORDS; c++) w[c] = sah_empty_word(c);
  }
}
__global__ void k_flags(int n, const int* __restrict__ prims, const int* __restrict__ node_of, const tnode* __restrict__ nodes,
    const float* __restrict__ ctr, int* flag) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  int f = 0;
  if (i < n) {
    int t = node_of[i];
    if (t >= 0 && nodes[t].swap) f = ctr[3 * prims[i] + nodes[t].axis] < nodes[t].split ? 1 : 0;
  }
  flag[i] = f;   // flag[n] = 0: the scan's last entry is the total
}
// split position and the two children of every internal node of the level
__global__ void k_children(int lb, int le, tnode* nodes, const int* __restrict__ tscan, int* counter) {
  int t = lb + blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= le) return;
  tnode& nd = nodes[t];
  if (nd.child == -1) return;
  if (nd.swap) {
    int mid = nd.start + (tscan[nd.end] - tscan[nd.start]);
    if (mid == nd.start || mid == nd.end) nd.swap = 0;   // :436: could not split: halves, nothing moved
    else nd.mid = mid;
  }
  int c = atomicAdd(counter, 2);
  nd.child = c;
  nodes[c]     = tnode{nd.start, nd.mid, t, 0, -1, 0, 0, 0, 0.0f, 0, 0};
  nodes[c + 1] = tnode{nd.mid, nd.end, t, 1, -1, 0, 0, 0, 0.0f, 0, 0};
}
// std::partition, step 1: every passing element right of the split position notes where it is, by its rank from the right
__global__ void k_partners(int n, const int* __restrict__ node_of, const tnode* __restrict__ nodes, const int* __restrict__ flag,
    const int* __restrict__ tscan, int* partner) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int t = node_of[i];
  if (t < 0 || !nodes[t].swap) return;
  const tnode& nd = nodes[t];
  if (i >= nd.mid && flag[i]) partner[nd.start + (tscan[nd.end] - tscan[i + 1])] = i;
}
// step 2: every failing element left of the split position swaps with the passing element of its rank; then every
// position learns which child it now belongs to
__global__ void k_swap(int n, int* prims, int* node_of, const tnode* __restrict__ nodes, const int* __restrict__ flag,
    const int* __restrict__ tscan, const int* __restrict__ partner) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int t = node_of[i];
  if (t < 0) return;
  const tnode& nd = nodes[t];
  if (nd.swap && i < nd.mid && !flag[i]) {
    int k = (i - nd.start) - (tscan[i] - tscan[nd.start]);
    int j = partner[nd.start + k];
    int a = prims[i];
    prims[i] = prims[j], prims[j] = a;
  }
  node_of[i] = nd.child < 0 ? -1 : (i < nd.mid ? nd.child : nd.child + 1);
}
__global__ void k_icount(int lb, int le, tnode* nodes) {
  int t = lb + blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= le) return;
  tnode& nd = nodes[t];
  nd.icount = nd.child < 0 ? 0 : 1 + nodes[nd.child].icount + nodes[nd.child + 1].icount;
}
__global__ void k_pre(int lb, int le, tnode* nodes) {
  int t = lb + blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= le) return;
  const tnode& nd = nodes[t];
  if (nd.child < 0) return;
  nodes[nd.child + 1].pre = nd.pre + 1;
  nodes[nd.child].pre     = nd.pre + 1 + nodes[nd.child + 1].icount;
}
__global__ void k_emit(int count, const tnode* __restrict__ nodes, const float* __restrict__ boxes, vpt_bvh_node* out) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const tnode& nd = nodes[t];
  int id = nd.parent < 0 ? 0 : 1 + 2 * nodes[nd.parent].pre + nd.which;
  vpt_bvh_node o;
  for (int c = 0; c < 3; c++) o.bbox_min[c] = boxes[6 * t + c], o.bbox_max[c] = boxes[6 * t + 3 + c];
  if (nd.child >= 0) o.start = 1 + 2 * nd.pre, o.num = 2, o.axis = (int8_t)nd.axis, o.internal = 1;
  else o.start = nd.start, o.num = (int16_t)(nd.end - nd.start), o.axis = 0, o.internal = 0;
  out[id] = o;
}

vpt_bvh_node empty_root() {   // the reference's root of an empty build: an invalid box, a leaf without primitives
  vpt_bvh_node o;
  for (int c = 0; c < 3; c++) o.bbox_min[c] = 3.402823466e+38f, o.bbox_max[c] = -3.402823466e+38f;
  o.start = 0, o.num = 0, o.axis = 0, o.internal = 0;
  return o;
}

}  // namespace

int bvh_build_scratch::reserve(int max_boxes, int quality) {
  if (quality == VPT_BVH_SAH && max_boxes > sah_reserved) {
    sah_reserved = -1;
    const size_t n = (size_t)(max_boxes > 0 ? max_boxes : 1), slots = n / (BVH_MAX_PRIMS + 1) + 1;
    if (sah_bins.allocate(slots * SAH_SLOT_WORDS * sizeof(unsigned)) || sah_info.allocate(slots * sizeof(sah_node_info)) || sah_slot.allocate(2 * n * sizeof(int)))
      return VPT_ERR_HIP;
    sah_reserved = max_boxes;
  }
  if (max_boxes <= reserved) return VPT_OK;
  reserved = -1;
  const size_t n = (size_t)(max_boxes > 0 ? max_boxes : 1), cap = 2 * n;
  if (ctr.allocate(3 * n * sizeof(float)) || boxes.allocate(6 * cap * sizeof(float)) || prims.allocate(n * sizeof(int)) || node_of.allocate(n * sizeof(int)) ||
      flag.allocate((n + 1) * sizeof(int)) || tscan.allocate((n + 1) * sizeof(int)) || partner.allocate(n * sizeof(int)) || counter.allocate(sizeof(int)) ||
      tnodes.allocate(cap * sizeof(tnode)) || keys.allocate(cap * sizeof(tkeys)) || out.allocate(cap * sizeof(vpt_bvh_node)))
    return VPT_ERR_HIP;
  scan_bytes = 0;   // of the largest scan; rocPRIM's need does not shrink with the size
  HIP_TRY(rocprim::exclusive_scan((void*)nullptr, scan_bytes, flag.get<int>(), tscan.get<int>(), 0, n + 1, rocprim::plus<int>()));
  if (int rc = scan_temp.allocate(scan_bytes)) return rc;
  reserved = max_boxes;
  return VPT_OK;
}

int bvh_build_core(bvh_build_scratch& s, const float* bb, int stride, int n, int* count_out, int* launches, int quality) {
  if (n < 0 || stride < 6 || !count_out || (n > 0 && !bb)) return vpt_set_error(VPT_ERR_INVALID_ARG, "bad argument");
  if (quality != VPT_BVH_MIDDLE && quality != VPT_BVH_SAH) return vpt_set_error(VPT_ERR_INVALID_ARG, "unknown bvh quality %d", quality);
  if (int rc = s.reserve(n, quality)) return rc;
  vpt_bvh_node* out = s.out.get<vpt_bvh_node>();
  if (n == 0) {
    const vpt_bvh_node o = empty_root();
    HIP_TRY(hipMemcpy(out, &o, sizeof(o), hipMemcpyHostToDevice));
    *count_out = 1;
    return VPT_OK;
  }
  const size_t cap = 2 * (size_t)n;
  float *ctr = s.ctr.get<float>(), *boxes = s.boxes.get<float>();
  int *  prims = s.prims.get<int>(), *node_of = s.node_of.get<int>(), *flag = s.flag.get<int>(), *tscan = s.tscan.get<int>(), *partner = s.partner.get<int>(), *counter = s.counter.get<int>();
  tnode* nodes = s.tnodes.get<tnode>();
  tkeys* keys  = s.keys.get<tkeys>();
  char*  scan_temp = s.scan_temp.get<char>();
  size_t scan_bytes = s.scan_bytes;
  int    launched = 0;

  const int  TB = 256;
  const dim3 gn((n + TB - 1) / TB), gn1((n + 1 + TB - 1) / TB);
  auto blocks = [&](int count) { return dim3((count + TB - 1) / TB); };
  hipLaunchKernelGGL(k_centers, gn, dim3(TB), 0, 0, n, bb, stride, ctr);
  hipLaunchKernelGGL(k_init, gn, dim3(TB), 0, 0, n, prims, node_of);
  launched += 2;
  const bool sah = quality == VPT_BVH_SAH;
  unsigned*  sah_bins = sah ? s.sah_bins.get<unsigned>() : nullptr;
  sah_node_info* sah_inf = sah ? s.sah_info.get<sah_node_info>() : nullptr;
  int*       sah_slot = sah ? s.sah_slot.get<int>() : nullptr;
  if (sah) {
    const size_t words = ((size_t)n / (BVH_MAX_PRIMS + 1) + 1) * SAH_SLOT_WORDS;   // the slots this build can name
    hipLaunchKernelGGL(k_sah_clear, dim3((unsigned)((words + TB - 1) / TB)), dim3(TB), 0, 0, words, sah_bins);
    launched++;
  }
  tnode root = {0, n, -1, 0, -1, 0, 0, 0, 0.0f, 0, 0};
  HIP_TRY(hipMemcpy(nodes, &root, sizeof(root), hipMemcpyHostToDevice));
  int count = 1;
  HIP_TRY(hipMemcpy(counter, &count, 4, hipMemcpyHostToDevice));

  std::vector<int> level_begin = {0};
  int lb = 0, le = 1;
  while (lb < le) {
    if (level_begin.size() > 4096) return vpt_set_error(VPT_ERR_HIP, "BVH build did not terminate");
    int ln = le - lb;
    hipLaunchKernelGGL(k_reset_keys, blocks(ln), dim3(TB), 0, 0, lb, le, keys);
    hipLaunchKernelGGL(k_bounds, gn, dim3(TB), 0, 0, n, prims, node_of, bb, stride, ctr, keys);
    if (sah) {
      hipLaunchKernelGGL(k_sah_prepare, blocks(ln), dim3(TB), 0, 0, lb, le, nodes, keys, prims, ctr, sah_slot, sah_inf);
      hipLaunchKernelGGL(k_sah_bin, gn, dim3(TB), 0, 0, n, prims, node_of, sah_slot, sah_inf, bb, stride, ctr, sah_bins);
      hipLaunchKernelGGL(k_decide_sah, dim3(ln), dim3(64), 0, 0, lb, le, nodes, keys, prims, bb, stride, ctr, boxes, sah_slot, sah_inf, sah_bins);
      launched += 2;
    } else
      hipLaunchKernelGGL(k_decide, blocks(ln), dim3(TB), 0, 0, lb, le, nodes, keys, prims, bb, stride, ctr, boxes);
    hipLaunchKernelGGL(k_flags, gn1, dim3(TB), 0, 0, n, prims, node_of, nodes, ctr, flag);
    HIP_TRY(rocprim::exclusive_scan((void*)scan_temp, scan_bytes, flag, tscan, 0, (size_t)n + 1, rocprim::plus<int>()));
    hipLaunchKernelGGL(k_children, blocks(ln), dim3(TB), 0, 0, lb, le, nodes, tscan, counter);
    hipLaunchKernelGGL(k_partners, gn, dim3(TB), 0, 0, n, node_of, nodes, flag, tscan, partner);
    hipLaunchKernelGGL(k_swap, gn, dim3(TB), 0, 0, n, prims, node_of, nodes, flag, tscan, partner);
    launched += 8;   // (the scan counted as one)
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&count, counter, 4, hipMemcpyDeviceToHost));   // also the level's barrier for the host
    if (count < le || (size_t)count > cap) return vpt_set_error(VPT_ERR_HIP, "BVH build produced %d nodes for %d primitives", count, n);
    lb = le, le = count;
    level_begin.push_back(lb);
  }
  // level_begin = starts of the levels, the last entry = count
  const int nlevels = (int)level_begin.size() - 1;
  for (int l = nlevels - 1; l >= 0; l--) {
    int a = level_begin[l], b = level_begin[l + 1];
    if (b <= a) continue;
    hipLaunchKernelGGL(k_icount, blocks(b - a), dim3(TB), 0, 0, a, b, nodes);
    launched++;
  }
  for (int l = 0; l < nlevels; l++) {
    int a = level_begin[l], b = level_begin[l + 1];
    if (b <= a) continue;
    hipLaunchKernelGGL(k_pre, blocks(b - a), dim3(TB), 0, 0, a, b, nodes);
    launched++;
  }
  hipLaunchKernelGGL(k_emit, blocks(count), dim3(TB), 0, 0, count, nodes, boxes, out);
  launched++;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  *count_out = count;
  if (launches) *launches += launched;
  return VPT_OK;
}

extern "C" int vpt_build_bvh(int device, const float* bboxes, int n, vpt_bvh_node* nodes_out, int capacity, int* num_nodes, int* primitives) {
  return vpt_build_bvh_quality(device, bboxes, n, VPT_BVH_MIDDLE, nodes_out, capacity, num_nodes, primitives);
}
extern "C" int vpt_build_bvh_quality(int device, const float* bboxes, int n, int quality, vpt_bvh_node* nodes_out, int capacity, int* num_nodes, int* primitives) {
  if (quality != VPT_BVH_MIDDLE && quality != VPT_BVH_SAH) return vpt_set_error(VPT_ERR_INVALID_ARG, "unknown bvh quality %d", quality);
  if (n < 0 || !nodes_out || !num_nodes || (n > 0 && (!bboxes || !primitives))) return vpt_set_error(VPT_ERR_INVALID_ARG, "bad argument");
  if (capacity < (n > 0 ? 2 * n - 1 : 1)) return vpt_set_error(VPT_ERR_INVALID_ARG, "node capacity %d < %d (2 n - 1)", capacity, n > 0 ? 2 * n - 1 : 1);
  if (n == 0) {
    nodes_out[0] = empty_root(), *num_nodes = 1;
    return VPT_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return vpt_set_error(VPT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return vpt_set_error(VPT_ERR_INVALID_ARG, "device %d out of range (%d devices)", device, ndev);
  HIP_TRY(hipSetDevice(device));

  device_buffer     d_bb;   // freed, like the scratch, on every exit path
  bvh_build_scratch s;
  if (int rc = d_bb.allocate(6 * (size_t)n * sizeof(float))) return rc;
  if (int rc = s.reserve(n, quality)) return rc;
  HIP_TRY(hipMemcpy(d_bb.get(), bboxes, 6 * (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  int count = 0;
  if (int rc = bvh_build_core(s, d_bb.get<float>(), 6, n, &count, nullptr, quality)) return rc;
  HIP_TRY(hipMemcpy(nodes_out, s.nodes(), (size_t)count * sizeof(vpt_bvh_node), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(primitives, s.primitives(), (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  *num_nodes = count;
  return VPT_OK;
}
