// Guided decoding for gfx950: a byte DFA per constrained sequence masks the fp32 copy of its
// logits row (the penalty slot's row, penalties.hip) before the sampler reads it, and follows the
// sampled id afterwards -- both inside the decode graphs, so the host never sees a step.
//
// State (ops/grammar.py; the layout and the semantics are written once in ops/reference.py):
//  * pool [n_tables, kTableWords] int32: one DFA per entry: [0] states S, [1] byte classes C,
//    [4:68] the class of every byte (256 x uint8), [68:132] one accept bit per state, then
//    trans[S][C] as int16 (-1 = DEAD).  An entry whose S or C is out of range is no table.
//  * rec [n_slots, kSlotWords] int32: table entry (-1 = none), state (-1 = DEAD), number of end
//    ids, 17 end ids.  The slot index is the penalty slot's.
//  * off int32 [V + 1] / bytes uint8 [n_bytes]: the byte string of every vocabulary id.
// mask, per id t < V of a row whose slot holds a table: an end id is kept iff the state accepts
// (at DEAD end ids are kept); an id with no bytes is dropped; any other id is kept iff its bytes
// never leave the automaton.  Dropped = -inf is stored; a kept word is not written at all.
// Every kernel returns early for a slot outside [0, n_slots) or without a table, and every index
// read from memory (state, class, next state, byte offsets) is range-checked before it is used.
#include "common.h"

using namespace pk;

namespace {

constexpr int kMaxStates = 2048;
constexpr int kMaxEnd = 17;
constexpr int kHeadWords = 132;
constexpr int kTableWords = kHeadWords + kMaxStates * 256 / 2;
constexpr int kSlotWords = 3 + kMaxEnd;
constexpr int kSeedWords = 4 + kMaxEnd;
constexpr int kThreads = 256;
constexpr int kMaskChunks = 8;  // workgroups per row: 8 x 256 threads walk a 128k vocabulary, 63 ids each

struct Table {
  const uint8_t* cmap;
  const uint32_t* accept;
  const int16_t* trans;
  int S, C;
};

// The table of a slot record, or S = 0 when the record names none.
__device__ __forceinline__ Table table_of(const int* __restrict__ pool, int n_tables, int tab) {
  Table t{nullptr, nullptr, nullptr, 0, 0};
  if (tab < 0 || tab >= n_tables) return t;
  const int* w = pool + static_cast<int64_t>(tab) * kTableWords;
  const int S = w[0], C = w[1];
  if (S < 1 || S > kMaxStates || C < 1 || C > 256) return t;
  t.cmap = reinterpret_cast<const uint8_t*>(w + 4);
  t.accept = reinterpret_cast<const uint32_t*>(w + 68);
  t.trans = reinterpret_cast<const int16_t*>(w + kHeadWords);
  t.S = S;
  t.C = C;
  return t;
}

// state after the bytes [b, e) from `state` (-1 = DEAD)
__device__ __forceinline__ int walk(const Table& t, int state, const uint8_t* __restrict__ bytes, int b, int e) {
  for (int i = b; i < e && state >= 0; ++i) {
    const int c = t.cmap[bytes[i]];
    int nxt = c < t.C ? t.trans[state * t.C + c] : -1;
    if (nxt >= t.S) nxt = -1;
    state = nxt;
  }
  return state;
}

__global__ void __launch_bounds__(kThreads) mask_kernel(float* __restrict__ out, int64_t ostride, int V,
                                                        const int* __restrict__ pool, int n_tables,
                                                        const int* __restrict__ rec, int n_slots,
                                                        const int* __restrict__ slots, const int* __restrict__ off,
                                                        const uint8_t* __restrict__ bytes, int n_bytes) {
  const int slot = slots[blockIdx.y];
  if (slot < 0 || slot >= n_slots) return;
  const int* r = rec + slot * kSlotWords;
  const Table t = table_of(pool, n_tables, r[0]);
  if (t.S == 0) return;
  int state = r[1];
  if (state < 0 || state >= t.S) state = -1;
  const int n_end = min(max(r[2], 0), kMaxEnd);
  const bool end_ok = state < 0 || ((t.accept[state >> 5] >> (state & 31)) & 1u);
  float* o = out + slot * ostride;
  for (int id = blockIdx.x * kThreads + threadIdx.x; id < V; id += gridDim.x * kThreads) {
    bool is_end = false;
    for (int j = 0; j < n_end; ++j) is_end |= r[3 + j] == id;
    bool keep;
    if (is_end) {
      keep = end_ok;
    } else {
      const int b = max(off[id], 0), e = min(off[id + 1], n_bytes);
      keep = e > b && walk(t, state, bytes, b, e) >= 0;
    }
    if (!keep) o[id] = -INFINITY;
  }
}

// one thread per batch row
__global__ void __launch_bounds__(kThreads) advance_kernel(const int* __restrict__ pool, int n_tables,
                                                           int* __restrict__ rec, int n_slots,
                                                           const int* __restrict__ slots,
                                                           const int* __restrict__ tokens, int B,
                                                           const int* __restrict__ off,
                                                           const uint8_t* __restrict__ bytes, int n_bytes, int V) {
  const int row = blockIdx.x * kThreads + threadIdx.x;
  if (row >= B) return;
  const int slot = slots[row];
  if (slot < 0 || slot >= n_slots) return;
  int* r = rec + slot * kSlotWords;
  const Table t = table_of(pool, n_tables, r[0]);
  const int id = tokens[row];
  if (t.S == 0 || id < 0 || id >= V) return;
  const int n_end = min(max(r[2], 0), kMaxEnd);
  for (int j = 0; j < n_end; ++j)
    if (r[3 + j] == id) return;  // the sequence stops on this id: the state stays
  int state = r[1];
  if (state < 0 || state >= t.S) state = -1;
  r[1] = walk(t, state, bytes, max(off[id], 0), min(off[id + 1], n_bytes));
}

__global__ void __launch_bounds__(kThreads) load_kernel(int* __restrict__ dst, const int* __restrict__ src, int n) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// one thread per entry
__global__ void __launch_bounds__(kThreads) seed_kernel(int* __restrict__ rec, int n_slots,
                                                        const int* __restrict__ entries, int n_entries) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_entries) return;
  const int* e = entries + i * kSeedWords;
  const int slot = e[0];
  if (slot < 0 || slot >= n_slots) return;
  for (int j = 0; j < kSlotWords; ++j) rec[slot * kSlotWords + j] = e[1 + j];
}

}  // namespace

// pool[entry][word_off : word_off + n_words] <- words (a table, or a chunk of one).  Eager only.
PK_EXPORT int pk_grammar_load(void* pool, int n_tables, int entry, int word_off, const void* words, int n_words,
                              hipStream_t stream) {
  if (n_words <= 0) return 0;
  if (n_tables <= 0 || entry < 0 || entry >= n_tables || word_off < 0 ||
      static_cast<int64_t>(word_off) + n_words > kTableWords)
    return -1;
  int* dst = static_cast<int*>(pool) + static_cast<int64_t>(entry) * kTableWords + word_off;
  load_kernel<<<(n_words + kThreads - 1) / kThreads, kThreads, 0, stream>>>(dst, static_cast<const int*>(words),
                                                                            n_words);
  return PK_CHECK_LAUNCH();
}

// entries int[n_entries, 21] = (slot, table entry, state, number of end ids, 17 end ids) -> slot
// records.  Entries of one launch name distinct slots.  Eager only.
PK_EXPORT int pk_grammar_seed(void* rec, int n_slots, const void* entries, int n_entries, hipStream_t stream) {
  if (n_entries <= 0) return 0;
  if (n_slots <= 0) return -1;
  seed_kernel<<<(n_entries + kThreads - 1) / kThreads, kThreads, 0, stream>>>(
      static_cast<int*>(rec), n_slots, static_cast<const int*>(entries), n_entries);
  return PK_CHECK_LAUNCH();
}

// out fp32 [n_slots, ostride]: -inf into every id < V the automaton of slots[row] does not admit,
// for every batch row < B whose slot holds a table.  off int32 [V + 1], bytes uint8 [n_bytes].
PK_EXPORT int pk_grammar_mask(void* out, int64_t ostride, int B, int V, const void* pool, int n_tables,
                              const void* rec, int n_slots, const void* slots, const void* off, const void* bytes,
                              int n_bytes, hipStream_t stream) {
  if (B <= 0) return 0;
  if (V <= 0 || ostride < V || n_tables <= 0 || n_slots <= 0 || n_bytes < 0) return -1;
  const int chunks = min(kMaskChunks, (V + kThreads - 1) / kThreads);
  mask_kernel<<<dim3(chunks, B), kThreads, 0, stream>>>(
      static_cast<float*>(out), ostride, V, static_cast<const int*>(pool), n_tables, static_cast<const int*>(rec),
      n_slots, static_cast<const int*>(slots), static_cast<const int*>(off), static_cast<const uint8_t*>(bytes),
      n_bytes);
  return PK_CHECK_LAUNCH();
}

// rec[slots[row]].state follows tokens[row] for every batch row < B whose slot holds a table; an
// end id leaves it alone.
PK_EXPORT int pk_grammar_advance(const void* pool, int n_tables, void* rec, int n_slots, const void* slots,
                                 const void* tokens, int B, const void* off, const void* bytes, int n_bytes, int V,
                                 hipStream_t stream) {
  if (B <= 0) return 0;
  if (V <= 0 || n_tables <= 0 || n_slots <= 0 || n_bytes < 0) return -1;
  advance_kernel<<<(B + kThreads - 1) / kThreads, kThreads, 0, stream>>>(
      static_cast<const int*>(pool), n_tables, static_cast<int*>(rec), n_slots, static_cast<const int*>(slots),
      static_cast<const int*>(tokens), B, static_cast<const int*>(off), static_cast<const uint8_t*>(bytes), n_bytes,
      V);
  return PK_CHECK_LAUNCH();
}
