// libmsm_frmem.so's kernels on the CPU (tests/test_frmem_host.py): the plan of csrc/frmem_plan.h and the per-lane functions of csrc/frmem_kernels.h,
// run workgroup by workgroup, lane by lane and phase by phase -- a barrier of the kernel is the end of a loop over the lanes here, a ballot a loop
// over the 64 lanes of a wave.  Every array is a heap allocation of exactly the size the library gives it, so that AddressSanitizer sees any
// access out of range.
//
//   frmem_harness sort|access key_bytes key_bits n tile n_t outputs in out      in: the keys (n words of key_bytes)
//       outputs: a mask -- sort: 1 perm_out, 2 keys_out; access: 1 rank, 2 prev, 4 counts, 8 last
//   frmem_harness args                                                           the argument checks, one line "name verdict" each
// out: eight words (error word, levels, total, 0, distinct, 0, launches, 0), then the outputs that were asked for, which start as bytes 0xA5.  Exit
// status 0; 2 where the library would return MSM_HIP_ERR_INVALID_ARG after its launches; 14 where its argument checks refuse the call.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "frmem_kernels.h"
#include "frmem_plan.h"

using namespace frmem;

static std::vector<uint8_t> read_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) exit(10);
  std::vector<uint8_t> b;
  uint8_t buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + k);
  fclose(f);
  return b;
}

// tile_ranks of csrc/frmem_kernels.h: zero, then four rounds of ballots, ranks (barrier) and counts (barrier)
template <class KEY>
static void tile_ranks(uint32_t* cnt, std::vector<FrmLane<KEY>>& s) {
  for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) frm_zero(cnt, lane);
  for (uint32_t e = 0; e < FRMEM_PER_LANE; e++) {
    uint64_t peers[FRMEM_THREADS];
    for (uint32_t wave = 0; wave < FRMEM_WAVES; wave++) {
      uint64_t bal[FRMEM_DIGIT_BITS] = {0}, in = 0;
      for (uint32_t l = 0; l < FRMEM_WAVE; l++) {
        const FrmLane<KEY>& t = s[wave * FRMEM_WAVE + l];
        if (!(t.valid >> e & 1u)) continue;
        in |= (uint64_t)1 << l;
        for (uint32_t b = 0; b < FRMEM_DIGIT_BITS; b++)
          if (t.digit[e] >> b & 1u) bal[b] |= (uint64_t)1 << l;
      }
      for (uint32_t l = 0; l < FRMEM_WAVE; l++) peers[wave * FRMEM_WAVE + l] = frm_peers(bal, in, s[wave * FRMEM_WAVE + l].digit[e]);
    }
    for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) frm_rank(cnt, lane, e, peers[lane], s[lane]);
    for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) frm_count(cnt, lane, e, peers[lane], s[lane]);
  }
}

// the inclusive scan of a workgroup's lane sums: block_scan, a loop over the lanes per phase
static void block_scan(FrmNode* lds, const std::vector<FrmScanLane>& s) {
  for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) frm_put(lds, lane, s[lane]);
  for (uint32_t step = 0; step < FRMEM_SCAN_STEPS; step++) {
    FrmNode v[FRMEM_THREADS];
    for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) v[lane] = frm_peek(lds, lane, step);
    for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) frm_add(lds, lane, v[lane]);
  }
}

// enqueue_scan of csrc/frmem_host.h; nodes[l]: level l >= 1, of its exact size
template <int KIND, class KEY>
static int scan(void* leaf, std::vector<std::vector<FrmNode>>& nodes, const std::vector<size_t>& len, uint32_t* start, uint32_t* res, uint32_t res_at, uint32_t tile) {
  const size_t top = len.size() - 1;
  FrmNode lds[FRMEM_THREADS];
  std::vector<FrmScanLane> s(FRMEM_THREADS);
  int launches = 0;
  for (size_t l = 0; l < top; l++, launches++)
    for (size_t wg = 0; wg < len[l + 1]; wg++) {
      for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) {
        if (l == 0) frm_scan_load<KIND, KEY>(tile, leaf, len[0], wg, lane, s[lane]);
        else frm_scan_load<FRMEM_INNER, uint32_t>(tile, nodes[l].data(), len[l], wg, lane, s[lane]);
      }
      block_scan(lds, s);
      frm_store_sum(lds, nodes[l + 1].data(), wg, len[l + 1]);
    }
  for (size_t l = top + 1; l-- > 0; launches++) {
    const FrmNode* above = l == top ? nullptr : nodes[l + 1].data();
    const size_t tiles = l == top ? 1 : len[l + 1];
    for (size_t wg = 0; wg < tiles; wg++) {
      for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) {
        if (l == 0) frm_scan_load<KIND, KEY>(tile, leaf, len[0], wg, lane, s[lane]);
        else frm_scan_load<FRMEM_INNER, uint32_t>(tile, nodes[l].data(), len[l], wg, lane, s[lane]);
      }
      block_scan(lds, s);
      for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) {
        if (l == 0) frm_scan_store<KIND>(tile, lds, above, leaf, start, len[0], wg, lane, s[lane]);
        else frm_scan_store<FRMEM_INNER>(tile, lds, above, nodes[l].data(), nullptr, len[l], wg, lane, s[lane]);
      }
      if (!above) frm_store_total(lds, res, res_at);
    }
  }
  return launches;
}

static std::vector<std::vector<FrmNode>> level_nodes(const std::vector<size_t>& len) {
  std::vector<std::vector<FrmNode>> nodes(len.size());
  for (size_t l = 1; l < len.size(); l++) nodes[l].assign(len[l], FrmNode{0xdeadbeefu, 0xdeadbeefu});
  return nodes;
}

template <class KEY>
static int run(bool access, uint32_t key_bits, size_t n, uint32_t tile, size_t n_t, uint32_t mask, const std::vector<uint8_t>& in, const char* out_path) {
  std::vector<KEY> keys(n);
  if (n) memcpy(keys.data(), in.data(), n * sizeof(KEY));
  // the outputs, each of its exact size and absent where not asked for: sort perm, keys; access rank, prev, counts, last
  const size_t bytes[4] = {n * 4, access ? n * 4 : n * sizeof(KEY), access ? n_t * 4 : 0, access ? n_t * 4 : 0};
  std::vector<std::vector<uint8_t>> out(4);
  void* p[4];
  for (int k = 0; k < 4; k++) {
    if (mask >> k & 1u) out[k].assign(bytes[k] ? bytes[k] : 1, 0xA5);
    p[k] = mask >> k & 1u ? out[k].data() : nullptr;
  }
  if (access ? !access_args_ok(p[0], p[1], p[2], p[3], n_t, keys.data(), sizeof(KEY), key_bits, n) : !sort_args_ok(p[0], p[1], keys.data(), sizeof(KEY), key_bits, n)) return 14;
  const bool table = access && (p[2] || p[3]);
  if (!tile_ok(n, tile)) return 14;
  const Plan y = plan_call(n, sizeof(KEY), key_bits, tile, access, table);
  const uint64_t max_key = max_key_of(key_bits, table ? n_t : 0);
  std::vector<uint32_t> res(FRMEM_RESULT_WORDS, 0);
  // the scratch buffer in its parts
  std::vector<KEY> buf_keys[2];
  std::vector<uint32_t> buf_idx[2], hist(y.dlen[0], 0xdeadbeefu), start(access ? n : 0, 0xdeadbeefu);
  for (size_t b = 0; b < y.bufs; b++) buf_keys[b].assign(n, (KEY)0xdeadbeefu), buf_idx[b].assign(n, 0xdeadbeefu);
  std::vector<std::vector<FrmNode>> dnodes = level_nodes(y.dlen);
  uint32_t cnt[FRMEM_WAVES * FRMEM_DIGITS];
  std::vector<FrmLane<KEY>> s(FRMEM_THREADS);
  int launches = 0;
  for (uint32_t pass = 0; pass < y.passes; pass++) {
    const FrmemArgs g = plan_args(y, pass, max_key);
    const int from = src_buffer(pass), to = dst_buffer(pass);
    const KEY* src_keys = from < 0 ? keys.data() : buf_keys[from].data();
    const uint32_t* src_idx = from < 0 ? nullptr : buf_idx[from].data();
    const bool last = pass + 1 == y.passes && !access;
    KEY* dst_keys = last ? static_cast<KEY*>(p[1]) : buf_keys[to].data();
    uint32_t* dst_idx = last ? static_cast<uint32_t*>(p[0]) : buf_idx[to].data();
    for (size_t wg = 0; wg < y.tiles; wg++) {  // k_frmem_hist
      for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++)
        if (!frm_load<KEY>(g, src_keys, nullptr, wg, lane, s[lane])) res[FRMEM_RES_ERR] = 1u;
      tile_ranks(cnt, s);
      for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) frm_store_hist(g, cnt, hist.data(), wg, lane);
    }
    launches += 1 + scan<FRMEM_WORDS, uint32_t>(hist.data(), dnodes, y.dlen, nullptr, res.data(), FRMEM_RES_TOTAL, y.tile);
    launches++;
    for (size_t wg = 0; wg < y.tiles && !res[FRMEM_RES_ERR]; wg++) {  // k_frmem_scatter
      for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) frm_load<KEY>(g, src_keys, src_idx, wg, lane, s[lane]);
      tile_ranks(cnt, s);
      for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) frm_offsets(g, cnt, hist.data(), wg, lane);
      for (uint32_t lane = 0; lane < FRMEM_THREADS; lane++) frm_place<KEY>(g, cnt, dst_keys, dst_idx, lane, s[lane]);
    }
  }
  if (access) {
    const int at = dst_buffer(y.passes - 1);
    uint32_t* const w[4] = {static_cast<uint32_t*>(p[0]), static_cast<uint32_t*>(p[1]), static_cast<uint32_t*>(p[2]), static_cast<uint32_t*>(p[3])};
    if (y.table) {
      const uint32_t lanes = (uint32_t)((n_t + FRMEM_THREADS - 1) / FRMEM_THREADS) * FRMEM_THREADS;  // the whole grid, the lanes behind n_t included
      for (uint32_t j = 0; j < lanes; j++) frm_fill_lane(res.data(), w[2], w[3], (uint32_t)n_t, j);
      launches++;
    }
    std::vector<std::vector<FrmNode>> hnodes = level_nodes(y.hlen);
    launches += scan<FRMEM_HEADS, KEY>(buf_keys[at].data(), hnodes, y.hlen, start.data(), res.data(), FRMEM_RES_DISTINCT, y.tile);
    const uint32_t lanes = (uint32_t)((n + FRMEM_THREADS - 1) / FRMEM_THREADS) * FRMEM_THREADS;
    for (uint32_t k = 0; k < lanes; k++)
      frm_access_lane<KEY>((uint32_t)n, y.table ? (uint32_t)n_t : 0u, res.data(), buf_keys[at].data(), buf_idx[at].data(), start.data(), w[0], w[1], w[2], w[3], k);
    launches++;
  }
  if (launches != y.launches) return 15;
  res[1] = (uint32_t)y.levels, res[6] = (uint32_t)launches;
  FILE* f = fopen(out_path, "wb");
  if (!f) return 13;
  fwrite(res.data(), 4, res.size(), f);
  for (int k = 0; k < 4; k++)
    if (p[k] && bytes[k]) fwrite(out[k].data(), 1, bytes[k], f);
  fclose(f);
  return res[FRMEM_RES_ERR] ? 2 : 0;
}

// the argument checks on addresses that are never touched
static int args() {
  char* const base = reinterpret_cast<char*>((uintptr_t)1 << 30);
  void *P = base, *K = base + (1 << 20), *IN = base + (2 << 20), *R = base + (3 << 20), *V = base + (4 << 20), *C = base + (5 << 20), *L = base + (6 << 20);
  const size_t big = ((size_t)1 << 26) + 1;
#define SAY(name, v) printf("%s %d\n", name, (int)(v))
  SAY("sort", sort_args_ok(P, K, IN, 4, 32, 100));
  SAY("sort-no-keys-out", sort_args_ok(P, nullptr, IN, 8, 64, 100));
  SAY("sort-max", sort_args_ok(P, nullptr, base + ((size_t)1 << 29), 4, 1, big - 1));
  SAY("sort-n-0", sort_args_ok(P, K, IN, 4, 32, 0));
  SAY("sort-n-big", sort_args_ok(P, nullptr, base + ((size_t)1 << 29), 4, 32, big));
  SAY("sort-bytes-2", sort_args_ok(P, K, IN, 2, 16, 100));
  SAY("sort-bytes-16", sort_args_ok(P, K, IN, 16, 16, 100));
  SAY("sort-bits-0", sort_args_ok(P, K, IN, 4, 0, 100));
  SAY("sort-bits-33", sort_args_ok(P, K, IN, 4, 33, 100));
  SAY("sort-bits-65", sort_args_ok(P, K, IN, 8, 65, 100));
  SAY("sort-null-perm", sort_args_ok(nullptr, K, IN, 4, 32, 100));
  SAY("sort-null-keys", sort_args_ok(P, K, nullptr, 4, 32, 100));
  SAY("sort-perm-in-keys", sort_args_ok(static_cast<char*>(IN) + 396, K, IN, 4, 32, 100));
  SAY("sort-perm-behind-keys", sort_args_ok(static_cast<char*>(IN) + 400, K, IN, 4, 32, 100));
  SAY("sort-keys-out-in-keys", sort_args_ok(P, static_cast<char*>(IN) - 396, IN, 4, 32, 100));
  SAY("sort-perm-in-keys-out", sort_args_ok(static_cast<char*>(K) + 796, K, IN, 8, 64, 100));
  SAY("sort-perm-misaligned", sort_args_ok(static_cast<char*>(P) + 2, K, IN, 4, 32, 100));
  SAY("sort-keys-misaligned", sort_args_ok(P, K, static_cast<char*>(IN) + 4, 8, 64, 100));
  SAY("access", access_args_ok(R, V, C, L, 50, IN, 4, 32, 100));
  SAY("access-rank-only", access_args_ok(R, nullptr, nullptr, nullptr, 0, IN, 4, 32, 100));
  SAY("access-last-only", access_args_ok(nullptr, nullptr, nullptr, L, 1, IN, 8, 40, 100));
  SAY("access-all-null", access_args_ok(nullptr, nullptr, nullptr, nullptr, 50, IN, 4, 32, 100));
  SAY("access-table-0", access_args_ok(R, V, C, L, 0, IN, 4, 32, 100));
  SAY("access-table-big", access_args_ok(R, nullptr, base + ((size_t)1 << 29), nullptr, big, IN, 4, 32, 100));
  SAY("access-table-ignored", access_args_ok(R, V, nullptr, nullptr, big, IN, 4, 32, 100));
  SAY("access-n-0", access_args_ok(R, V, C, L, 50, IN, 4, 32, 0));
  SAY("access-bits-0", access_args_ok(R, V, C, L, 50, IN, 4, 0, 100));
  SAY("access-bytes-3", access_args_ok(R, V, C, L, 50, IN, 3, 8, 100));
  SAY("access-null-keys", access_args_ok(R, V, C, L, 50, nullptr, 4, 32, 100));
  SAY("access-rank-is-prev", access_args_ok(R, R, C, L, 50, IN, 4, 32, 100));
  SAY("access-counts-in-last", access_args_ok(R, V, static_cast<char*>(L) + 196, L, 50, IN, 4, 32, 100));
  SAY("access-counts-behind-last", access_args_ok(R, V, static_cast<char*>(L) + 200, L, 50, IN, 4, 32, 100));
  SAY("access-prev-in-keys", access_args_ok(R, static_cast<char*>(IN) + 4, C, L, 50, IN, 4, 32, 100));
  SAY("access-last-in-rank", access_args_ok(R, V, C, static_cast<char*>(R) - 196, 50, IN, 4, 32, 100));
  SAY("access-rank-misaligned", access_args_ok(static_cast<char*>(R) + 1, V, C, L, 50, IN, 4, 32, 100));
  SAY("tile-5-at-the-largest-n", tile_ok((size_t)1 << 26, 5));
  SAY("tile-4-at-the-largest-n", tile_ok((size_t)1 << 26, 4));
  SAY("tile-2-at-2^24", tile_ok((size_t)1 << 24, 2));
#undef SAY
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "args") return args();
  if (argc != 10) return 11;
  const std::string cmd = argv[1];
  if (cmd != "sort" && cmd != "access") return 11;
  const size_t key_bytes = strtoull(argv[2], nullptr, 10), n = strtoull(argv[4], nullptr, 10), n_t = strtoull(argv[6], nullptr, 10);
  const uint32_t key_bits = (uint32_t)strtoul(argv[3], nullptr, 10), tile = tile_of((uint32_t)strtoul(argv[5], nullptr, 10)), mask = (uint32_t)strtoul(argv[7], nullptr, 10);
  if (key_bytes != 4 && key_bytes != 8) return 14;
  if (n > MAX_ELEMENTS) return 14;  // (nothing of that size is allocated here)
  const std::vector<uint8_t> in = read_file(argv[8]);
  if (in.size() != n * key_bytes) return 12;
  return key_bytes == 4 ? run<uint32_t>(cmd == "access", key_bits, n, tile, n_t, mask, in, argv[9]) : run<uint64_t>(cmd == "access", key_bits, n, tile, n_t, mask, in, argv[9]);
}
