// Device side of ReplayBufferNoResampling (the reference's
// replay_buffer_no_resampling.py:8-173), the use-once buffer of
// --no_resampling: every transition is drawn exactly once and its slot is then
// handed to the next insert.
//
// Device state (all int32, owned by the caller):
//   valid[2][capacity]  the ordered list of live slots (_valid_indeces); a take
//                       reads one buffer and writes the other, the host swaps
//   queue[capacity]     the ring of freed slots (indices_to_replace)
// The host keeps every length and counter (they follow from call counts), so
// grids are sized on the host and nothing is read back.
//
// * take (random_batch, :124-141 and add_indices_to_replace, :91-96): B distinct
//   POSITIONS of the list -> idx[b] = valid_in[pos[b]] in draw order,
//   queue[(top_indexes + b) % capacity] = idx[b], and valid_out = the list
//   without those positions, order kept.  Two launches: one workgroup draws (or
//   loads) the positions, gathers, sorts the positions in LDS (bitonic) and
//   stores shift[m] = sorted[m] - m; then every output element k binary-searches
//   s = #{m : shift[m] <= k} and copies valid_in[k + s].
// * position draw (index_source='device'): Floyd's subset sampling on Philox.
//   Step t = 0 .. B-1, j = n - B + t:  words {t, 4, d lo, d hi} under the seed,
//   w = (word0 << 32) | word1, r = mulhi64(w, j + 1), pick_t = r unless r is
//   among pick_0 .. pick_{t-1}, then j.  No rejection loop; bias <= (j+1)/2^64.
//   Parallel form with the same picks: step t collides iff an earlier step drew
//   the same r, or r == j_s for an earlier step s that collided itself (then
//   pick_s = j_s); the second is a chain s < t, walked by each thread.
// * insert (add_sample, :98-122): replay_insert_kernel's packing with a slot
//   indirection, slot(s) = s < q ? queue[(bottom + s) % capacity]
//                                : (top + s - q) % capacity,
//   and valid[len + s] = slot(s) in the same launch.
//
// Integer only, no atomics, no cross-workgroup hand-off; every loop is bounded
// by B, the padded B's log2 or a grid stride.
#include <hip/hip_runtime.h>

#include <atomic>
#include <climits>

#include "kernels.h"
#include "oac_common.h"

namespace oac {

constexpr int kNrMaxB = 4096;        // positions per take (LDS sort)
constexpr int kNrChunk = 256;        // list elements per compaction workgroup
constexpr unsigned kNrStream = 4u;   // Philox stream id (1, 2: policy noise, 3: taken)

static std::atomic<long long> g_nr_launches{0};

struct NrTakeArgs {
  const int* valid_in; long len;        // live list and its length
  const int* positions;                 // [B] device, or null: draw them
  int B;
  int* queue; long capacity, top_idx;   // freed-slot ring and _top_indexes
  int* idx_out;                         // [B] drawn slots, draw order
  int* pos_out;                         // [B] the positions used (may be null)
  int* shift;                           // [B] sorted[m] - m for the compaction
  unsigned long long seed, draw;        // Philox key and draw counter
};

// B picks of Floyd's sampling from [0, n) into pos[0:B] (LDS), all 1024 threads
__device__ __forceinline__ void nr_floyd_draw(int* pos, unsigned char* col, long n, int B,
                                              unsigned long long seed, unsigned long long d) {
  const int tid = threadIdx.x;
  const long base = n - B;   // j_t = base + t
  for (int t = tid; t < B; t += 1024) {
    unsigned c[4] = {(unsigned)t, kNrStream, (unsigned)d, (unsigned)(d >> 32)};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    const unsigned long long w = ((unsigned long long)c[0] << 32) | c[1];
    pos[t] = (int)__umul64hi(w, (unsigned long long)(base + t + 1));
  }
  __syncthreads();
  for (int t = tid; t < B; t += 1024) {   // an earlier step drew the same r
    const int rt = pos[t];
    bool dup = false;
    for (int s = 0; s < t; ++s) dup |= pos[s] == rt;
    col[t] = dup ? 1 : 0;
  }
  __syncthreads();
  int pick[kNrMaxB / 1024];
#pragma unroll
  for (int k = 0; k < kNrMaxB / 1024; ++k) {
    const int t = tid + k * 1024;
    pick[k] = 0;
    if (t < B) {
      bool hit = false;
      int cur = t;
      for (int it = 0; it < B; ++it) {   // r == j_s of an earlier collided step s
        if (col[cur]) { hit = true; break; }
        const long s = (long)pos[cur] - base;
        if (s < 0 || s >= cur) break;
        cur = (int)s;
      }
      pick[k] = hit ? (int)(base + t) : pos[t];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kNrMaxB / 1024; ++k) {
    const int t = tid + k * 1024;
    if (t < B) pos[t] = pick[k];
  }
  __syncthreads();
}

__global__ void __launch_bounds__(1024) nr_positions_kernel(long n, int B, unsigned long long seed,
                                                           unsigned long long d, int* out) {
  __shared__ int pos[kNrMaxB];
  __shared__ unsigned char col[kNrMaxB];
  nr_floyd_draw(pos, col, n, B, seed, d);
  for (int t = threadIdx.x; t < B; t += 1024) out[t] = pos[t];
}

__global__ void __launch_bounds__(1024) nr_take_kernel(NrTakeArgs a) {
  __shared__ int pos[kNrMaxB];
  __shared__ unsigned char col[kNrMaxB];
  const int tid = threadIdx.x;
  const int B = a.B;
  if (a.positions) {
    for (int t = tid; t < B; t += 1024) {
      long p = a.positions[t];
      p = p < 0 ? 0 : (p >= a.len ? a.len - 1 : p);   // the host checked them; never read outside
      pos[t] = (int)p;
    }
    __syncthreads();
  } else {
    nr_floyd_draw(pos, col, a.len, B, a.seed, a.draw);
  }
  for (int t = tid; t < B; t += 1024) {
    const int v = a.valid_in[pos[t]];
    a.idx_out[t] = v;
    a.queue[(a.top_idx + t) % a.capacity] = v;
    if (a.pos_out) a.pos_out[t] = pos[t];
  }
  int P = 1;
  while (P < B) P <<= 1;
  for (int t = B + tid; t < P; t += 1024) pos[t] = INT_MAX;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {        // bitonic sort, ascending
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += 1024) {
        const int l = i ^ j;
        if (l > i) {
          const int x = pos[i], y = pos[l];
          const bool up = (i & k) == 0;
          if ((x > y) == up) { pos[i] = y; pos[l] = x; }
        }
      }
      __syncthreads();
    }
  }
  for (int m = tid; m < B; m += 1024) a.shift[m] = pos[m] - m;
}

__global__ void __launch_bounds__(kNrChunk) nr_compact_kernel(const int* valid_in, const int* shift,
                                                              int B, long out_len, int* valid_out) {
  const long k = (long)blockIdx.x * kNrChunk + threadIdx.x;
  if (k >= out_len) return;
  int lo = 0, hi = B;   // s = #{m : shift[m] <= k}: removed positions before output k's source
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (shift[mid] <= k) lo = mid + 1; else hi = mid;
  }
  valid_out[k] = valid_in[k + lo];
}

struct NrInsertArgs {
  ReplayInsertArgs r;                 // r.top = _top, r.n = rows
  const int* queue; long bottom;      // freed-slot ring and _bottom_indexes
  int q;                              // ring entries, as the reference's counters see them
  int* valid; long len;               // live list and its length before the insert
};

__global__ void __launch_bounds__(256) nr_insert_kernel(NrInsertArgs b) {
  const ReplayInsertArgs& a = b.r;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)a.n * a.row_stride;
  if (e >= total) return;
  const int i = (int)(e / a.row_stride);
  const int c = (int)(e - (long)i * a.row_stride);
  float v = 0.f;   // row padding stays zero
  if (c >= a.off_obs && c < a.off_obs + a.obs_dim) v = (float)a.obs[(long)i * a.obs_dim + c - a.off_obs];
  else if (c >= a.off_act && c < a.off_act + a.act_dim) v = (float)a.act[(long)i * a.act_dim + c - a.off_act];
  else if (c == a.off_rew) v = (float)a.rew[i];
  else if (c == a.off_term) v = a.term[i] ? 1.f : 0.f;
  else if (c >= a.off_next_obs && c < a.off_next_obs + a.obs_dim)
    v = (float)a.next_obs[(long)i * a.obs_dim + c - a.off_next_obs];
  const long row = i < b.q ? (long)b.queue[(b.bottom + i) % a.capacity]
                           : (a.top + i - b.q) % a.capacity;
  if (row < 0 || row >= a.capacity) return;   // a ring entry that is no slot: never write outside
  a.storage[row * a.row_stride + c] = v;
  if (c == 0) b.valid[b.len + i] = (int)row;
}

}  // namespace oac

using namespace oac;

extern "C" {

int64_t oac_replay_nr_chunk(void) { return kNrChunk; }

int64_t oac_replay_nr_launch_count(void) { return g_nr_launches.load(); }

static int nr_check_draw(const char* who, int64_t n, int B) {
  if (B < 1) { set_error("%s: B = %d < 1", who, B); return 1; }
  if (B > kNrMaxB) { set_error("%s: B = %d > %d (the positions are sorted in LDS)", who, B, kNrMaxB); return 1; }
  if (n >= (1LL << 31)) { set_error("%s: capacity %lld >= 2^31", who, (long long)n); return 1; }
  if ((int64_t)B > n) { set_error("%s: B = %d > len = %lld", who, B, (long long)n); return 1; }
  return 0;
}

int oac_replay_nr_sample_positions(int64_t n, int B, uint64_t seed, uint64_t draw_counter,
                                   int32_t* positions_out, void* stream) {
  if (nr_check_draw("replay_nr_sample_positions", n, B)) return 1;
  if (!positions_out) { set_error("replay_nr_sample_positions: null buffer"); return 1; }
  OAC_LAUNCH(nr_positions_kernel, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream),
             (long)n, B, (unsigned long long)seed, (unsigned long long)draw_counter, positions_out);
  g_nr_launches += 1;
  OAC_HIP_CHECK(hipGetLastError());
  return 0;
}

int oac_replay_nr_take(const int32_t* valid_in, int64_t len, const int32_t* positions, int B,
                       int32_t* queue, int64_t capacity, int64_t top_indexes, int32_t* idx_out,
                       int32_t* positions_out, int32_t* valid_out, int32_t* scratch, uint64_t seed,
                       uint64_t draw_counter, void* stream) {
  if (capacity >= (1LL << 31)) { set_error("replay_nr_take: capacity %lld >= 2^31", (long long)capacity); return 1; }
  if (nr_check_draw("replay_nr_take", len, B)) return 1;
  if (capacity < 1 || len > capacity || top_indexes < 0 || top_indexes >= capacity) {
    set_error("replay_nr_take: bad capacity / len / top_indexes");
    return 1;
  }
  if (!valid_in || !queue || !idx_out || !valid_out || !scratch) {
    set_error("replay_nr_take: null buffer");
    return 1;
  }
  if (valid_in == valid_out) { set_error("replay_nr_take: valid_out aliases valid_in"); return 1; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  NrTakeArgs a;
  a.valid_in = valid_in; a.len = len; a.positions = positions; a.B = B;
  a.queue = queue; a.capacity = capacity; a.top_idx = top_indexes;
  a.idx_out = idx_out; a.pos_out = positions_out; a.shift = scratch;
  a.seed = seed; a.draw = draw_counter;
  OAC_LAUNCH(nr_take_kernel, dim3(1), dim3(1024), 0, s, a);
  g_nr_launches += 1;
  const long out_len = (long)(len - B);
  if (out_len > 0) {
    OAC_LAUNCH(nr_compact_kernel, dim3((unsigned)((out_len + kNrChunk - 1) / kNrChunk)), dim3(kNrChunk),
               0, s, valid_in, (const int*)scratch, B, out_len, valid_out);
    g_nr_launches += 1;
  }
  OAC_HIP_CHECK(hipGetLastError());
  return 0;
}

int oac_replay_nr_insert(float* storage, int64_t row_stride, int64_t capacity, int64_t top,
                         const int32_t* queue, int64_t bottom_indexes, int64_t queue_entries,
                         int32_t* valid, int64_t len, int n, const double* obs, const double* act,
                         const double* rew, const double* next_obs, const uint8_t* term, int obs_dim,
                         int act_dim, int off_obs, int off_act, int off_rew, int off_term,
                         int off_next_obs, void* stream) {
  if (capacity >= (1LL << 31)) { set_error("replay_nr_insert: capacity %lld >= 2^31", (long long)capacity); return 1; }
  if (!storage || !queue || !valid) { set_error("replay_nr_insert: null buffer"); return 1; }
  if (capacity < 1 || top < 0 || top >= capacity || bottom_indexes < 0 || bottom_indexes >= capacity ||
      queue_entries < 0 || queue_entries >= capacity || n < 0 || len < 0) {
    set_error("replay_nr_insert: bad capacity / top / bottom_indexes / queue_entries / n");
    return 1;
  }
  if (len + n > capacity) {
    set_error("replay_nr_insert: len %lld + n %d > capacity %lld", (long long)len, n, (long long)capacity);
    return 1;
  }
  if (off_obs + obs_dim > row_stride || off_act + act_dim > row_stride || off_rew >= row_stride ||
      off_term >= row_stride || off_next_obs + obs_dim > row_stride) {
    set_error("replay_nr_insert: row layout out of bounds");
    return 1;
  }
  if (n == 0) return 0;
  if (!obs || !act || !rew || !next_obs || !term) { set_error("replay_nr_insert: null buffer"); return 1; }
  NrInsertArgs b;
  ReplayInsertArgs& a = b.r;
  a.storage = storage; a.row_stride = row_stride; a.capacity = capacity; a.top = top; a.n = n;
  a.obs = obs; a.act = act; a.rew = rew; a.next_obs = next_obs; a.term = term;
  a.obs_dim = obs_dim; a.act_dim = act_dim; a.off_obs = off_obs; a.off_act = off_act;
  a.off_rew = off_rew; a.off_term = off_term; a.off_next_obs = off_next_obs;
  b.queue = queue; b.bottom = bottom_indexes; b.q = (int)queue_entries; b.valid = valid; b.len = len;
  const long total = (long)n * row_stride;
  OAC_LAUNCH(nr_insert_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
             reinterpret_cast<hipStream_t>(stream), b);
  g_nr_launches += 1;
  OAC_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
