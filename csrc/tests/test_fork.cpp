// Host-side sanitizer test of BlockManagerCore::fork (built with -fsanitize=address,undefined and run
// by tests/unit/test_block_fork.py): random fork / free / allocate / commit / match churn under the
// invariants of test_native.cpp's prefix-cache churn, the shape of a fork's result, and the
// atomicity of every failing fork.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>

#include "runtime/block_manager.h"

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d CHECK(%s)\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

namespace {

struct Snapshot {
  int64_t free, cached, seqs;
  std::vector<int32_t> refs;
  std::map<int64_t, std::vector<int32_t>> tables;
  bool operator==(const Snapshot& o) const {
    return free == o.free && cached == o.cached && seqs == o.seqs && refs == o.refs && tables == o.tables;
  }
};

Snapshot snap(const pk::BlockManagerCore& bm, int64_t max_seq) {
  Snapshot s{bm.num_free(), bm.num_cached(), bm.num_seqs(), {}, {}};
  for (int64_t b = 0; b < bm.num_blocks(); ++b) s.refs.push_back(bm.ref_count(static_cast<int32_t>(b)));
  for (int64_t q = 0; q < max_seq; ++q)
    if (bm.has(q)) s.tables[q] = bm.table(q);
  return s;
}

// every ref count equals the number of tables holding the block; free + held == num_blocks
void check_invariants(const pk::BlockManagerCore& bm, const std::map<int64_t, int64_t>& len) {
  std::map<int32_t, int> refs;
  for (auto& kv : len) {
    CHECK(bm.has(kv.first));
    auto t = bm.table(kv.first);
    CHECK(static_cast<int64_t>(t.size()) >= bm.blocks_for(kv.second));
    std::set<int32_t> own;
    for (int32_t b : t) {
      CHECK(b >= 0 && b < bm.num_blocks());
      CHECK(own.insert(b).second);  // no block twice in one table
      ++refs[b];
    }
  }
  CHECK(bm.num_seqs() == static_cast<int64_t>(len.size()));
  for (int64_t b = 0; b < bm.num_blocks(); ++b) {
    auto it = refs.find(static_cast<int32_t>(b));
    CHECK(bm.ref_count(static_cast<int32_t>(b)) == (it == refs.end() ? 0 : it->second));
  }
  CHECK(static_cast<int64_t>(refs.size()) + bm.num_free() == bm.num_blocks());
}

void test_fork_shape() {
  const int BS = 8;
  pk::BlockManagerCore bm(8, BS, 0);
  std::vector<int32_t> pairs;
  CHECK(bm.allocate(1, 21));  // 3 blocks
  const auto src = bm.table(1);
  // 20 tokens: 2 shared blocks + 1 private, copied from src's block 2
  CHECK(bm.fork(1, 2, 20, &pairs));
  auto t = bm.table(2);
  CHECK(t.size() == 3 && t[0] == src[0] && t[1] == src[1] && t[2] != src[2]);
  CHECK(pairs.size() == 2 && pairs[0] == src[2] && pairs[1] == t[2]);
  CHECK(bm.ref_count(src[0]) == 2 && bm.ref_count(src[1]) == 2 && bm.ref_count(src[2]) == 1 && bm.ref_count(t[2]) == 1);
  CHECK(bm.num_free() == 4);
  // 16 tokens: a block boundary, nothing to copy
  CHECK(bm.fork(1, 3, 16, &pairs));
  CHECK(pairs.empty() && bm.table(3).size() == 2 && bm.ref_count(src[0]) == 3 && bm.num_free() == 4);
  // fewer than a block: only the private block
  CHECK(bm.fork(1, 4, 5, &pairs));
  CHECK(pairs.size() == 2 && pairs[0] == src[0] && bm.table(4).size() == 1 && bm.num_free() == 3);
  // the source may end first: the shared blocks live on with the fork
  bm.free_seq(1);
  CHECK(bm.ref_count(src[0]) == 2 && bm.ref_count(src[2]) == 0);
  CHECK(bm.allocate(2, 40));  // the fork grows like any sequence
  bm.free_seq(2);
  bm.free_seq(3);
  bm.free_seq(4);
  CHECK(bm.num_free() == 8 && bm.num_seqs() == 0);
}

void test_fork_failure_is_atomic() {
  const int BS = 8;
  pk::BlockManagerCore bm(6, BS, 0, true);
  std::vector<int32_t> pairs{7, 7};
  CHECK(bm.allocate(1, 20));  // 3 blocks
  CHECK(bm.allocate(2, 8));   // 1 block
  auto expect_refused = [&](int64_t src, int64_t dst, int64_t n) {
    const Snapshot before = snap(bm, 16);
    pairs = {7, 7};
    CHECK(!bm.fork(src, dst, n, &pairs));
    CHECK(pairs.empty());
    CHECK(snap(bm, 16) == before);
  };
  expect_refused(1, 2, 20);   // dst already has a table
  expect_refused(9, 3, 8);    // src missing
  expect_refused(1, 3, 25);   // src shorter than n_tokens
  expect_refused(1, 3, 0);    // nothing to fork
  expect_refused(1, 1, 8);    // onto itself
  CHECK(bm.allocate(4, 16));  // the pool is now full: 3 + 1 + 2
  CHECK(bm.num_free() == 0);
  expect_refused(1, 3, 20);   // no block for the remainder (and the 2 shared refs are not taken)
  CHECK(bm.fork(1, 3, 16, &pairs));  // a boundary fork needs no block
  CHECK(pairs.empty() && bm.num_free() == 0);
  for (int64_t s : {1, 2, 3, 4}) bm.free_seq(s);
  CHECK(bm.num_free() == 6 && bm.num_seqs() == 0);
}

void test_fork_churn() {
  const int64_t NB = 48;
  const int BS = 8;
  const int64_t NSEQ = 20;
  pk::BlockManagerCore bm(NB, BS, 0, true, 77);
  std::mt19937_64 rng(4321);
  std::vector<std::vector<uint64_t>> pref(3, std::vector<uint64_t>(4));
  std::vector<std::vector<int32_t>> ptoks(3, std::vector<int32_t>(4 * BS));
  for (int p = 0; p < 3; ++p) {
    for (int i = 0; i < 4 * BS; ++i) ptoks[p][i] = p * 1000 + (i % 5);
    CHECK(bm.prefix_hashes(ptoks[p].data(), 4 * BS, pref[p].data(), 4) == 4);
  }
  std::map<int64_t, int64_t> len;  // shadow: seq -> tokens its table covers
  std::map<int64_t, int> prompt;   // seq -> the prefix it was admitted with (forks: none)
  int forks = 0, refused = 0;
  std::vector<int32_t> pairs;
  for (int it = 0; it < 1000; ++it) {
    const int r = static_cast<int>(rng() % 8);  // 3 of 8 operations fork, 2 free: targets are often vacant
    const int op = r < 3 ? 0 : r < 5 ? 1 : r - 3;
    const int64_t seq = static_cast<int64_t>(rng() % NSEQ);
    if (op == 0) {  // fork a random prefix of a live sequence onto seq
      const int64_t src = static_cast<int64_t>(rng() % NSEQ);
      const int64_t n = static_cast<int64_t>(rng() % 40);
      const bool can = len.count(src) && !len.count(seq) && src != seq && n > 0 &&
                       bm.blocks_for(n) <= static_cast<int64_t>(bm.table(src).size()) &&
                       (n % BS == 0 || bm.num_free() > 0);
      const Snapshot before = snap(bm, NSEQ);
      const bool ok = bm.fork(src, seq, n, &pairs);
      CHECK(ok == can);
      if (ok) {
        ++forks;
        len[seq] = n;
        const auto s = bm.table(src), d = bm.table(seq);
        CHECK(static_cast<int64_t>(d.size()) == bm.blocks_for(n));
        for (int64_t i = 0; i < n / BS; ++i) CHECK(d[i] == s[i]);
        CHECK(pairs.size() == (n % BS ? 2u : 0u));
        if (n % BS) CHECK(pairs[0] == s[n / BS] && pairs[1] == d.back() && bm.ref_count(d.back()) == 1);
      } else {
        ++refused;
        CHECK(snap(bm, NSEQ) == before);
      }
    } else if (op == 1) {  // free
      bm.free_seq(seq);
      len.erase(seq);
      prompt.erase(seq);
    } else if (op == 2) {  // allocate / grow
      const int64_t total = (len.count(seq) ? len[seq] : 0) + 1 + static_cast<int64_t>(rng() % 30);
      if (bm.allocate(seq, total)) len[seq] = total;
    } else if (op == 3 && !len.count(seq)) {  // admit through the prefix cache
      const int p = static_cast<int>(rng() % 3);
      bm.match_prefix(seq, pref[p].data(), ptoks[p].data(), 4 * BS, 3);
      if (bm.allocate(seq, 4 * BS)) {
        len[seq] = 4 * BS;
        prompt[seq] = p;
      } else {
        bm.free_seq(seq);
      }
    } else if (op == 4 && prompt.count(seq)) {  // commit
      const int p = prompt[seq];
      bm.commit_prefix(seq, pref[p].data(), ptoks[p].data(), 4 * BS, 4);
    }
    check_invariants(bm, len);
  }
  std::printf("churn: %d forks, %d refused\n", forks, refused);
  CHECK(forks >= 40 && refused >= 40);
  for (auto& kv : len) bm.free_seq(kv.first);
  CHECK(bm.num_free() == NB && bm.num_seqs() == 0);
  bm.reset_prefix_cache();
  CHECK(bm.num_cached() == 0 && bm.num_free() == NB);
}

}  // namespace

int main() {
  test_fork_shape();
  test_fork_failure_is_atomic();
  test_fork_churn();
  if (g_fail) {
    std::fprintf(stderr, "%d fork checks failed\n", g_fail);
    return 1;
  }
  std::printf("fork tests OK\n");
  return 0;
}
