// Stand-alone host program for tests/test_frlook_host.py: libmsm_frlook.so's lookup run on the CPU -- the plan of csrc/frlook_plan.h (slot count,
// hash mask, 2^256 mod r) and, lane by lane in serial order, the very functions the kernels of csrc/frlook_kernels.h call, with the host
// definitions of the atomics shim.  Built with g++ -DFQ_CHECK, so the assertions of those functions (an occupant is a table index, the probe
// loop ends before the slots run out, a sum below 2^256, a count below 2^27) are on.
//   frlook_harness run <n_t> <hash_bits> <mont> <n> <batch> <stride> <in> <out>
//        in:  table[n_t x 32] f[batch x stride x 32]
//        out: eight words -- error word, distinct, missing (2), first_missing (2), slots, distinct by the plan's serial build -- then
//             slots[slots] counts[n_t] idx[batch x n] m[n_t x 32 bytes]
//   exit status: 0 ok, 3 an element of the table or of f that is read is not below r, 2 bad arguments
// Compile with -DMSM_FIELD_NS=frl_<name> -DMSM_CURVE_CONSTANTS="fr_<name>_constants.h".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include MSM_CURVE_CONSTANTS
#include "frlook_kernels.h"
#include "frlook_plan.h"

using namespace MSM_FIELD_NS;

static bool read_file(const char* path, std::vector<uint32_t>& out, size_t words) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  out.resize(words);
  const bool ok = words == 0 || fread(out.data(), 4, words, f) == words;
  fclose(f);
  return ok;
}
static bool write_file(const char* path, const std::vector<uint32_t>& words) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = words.empty() || fwrite(words.data(), 4, words.size(), f) == words.size();
  fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 10 || strcmp(argv[1], "run")) return 2;
  const size_t n_t = (size_t)atoll(argv[2]);
  const uint32_t hash_bits = (uint32_t)atoi(argv[3]);
  const bool mont = atoi(argv[4]) != 0;
  const size_t n = (size_t)atoll(argv[5]), batch = (size_t)atoll(argv[6]), stride = (size_t)atoll(argv[7]);
  if (!frlook::table_args_ok(n_t, mont ? frlook::FLAG_MONT256 : 0) || !frlook::count_args_ok(n, batch, stride) || hash_bits > 32) return 2;
  std::vector<uint32_t> in;
  if (!read_file(argv[8], in, (n_t + batch * stride) * 8)) return 2;
  const uint32_t* keys = in.data();
  const uint32_t* f = in.data() + n_t * 8;
  const host_fr::Field field(FQ_P32);
  const FrlookArgs g = frlook::plan_args(field, n_t, hash_bits, mont);
  const size_t slot_words = (size_t)g.slot_mask + 1, total = batch * n;

  std::vector<uint32_t> out(8 + slot_words + n_t + total + n_t * 8, 0xa5a5a5a5u);
  uint32_t* res = out.data();
  uint32_t* slots = res + 8;
  uint32_t* counts = slots + slot_words;
  uint32_t* idx = counts + n_t;
  std::vector<uint32_t> m(n_t * 8), work(n_t, 0);  // (m apart: its stores are 32 bytes wide)
  memset(res, 0, 32);
  memset(res + FRLOOK_RES_FIRST, 0xff, 8);
  for (size_t s = 0; s < slot_words; s++) slots[s] = FRLOOK_EMPTY;

  // k_frlook_build
  for (uint32_t j = 0; j < g.n_t; j++) {
    bool won = false;
    if (!frl_build_lane(g, keys, slots, j, won)) frl_atomic_or(res + FRLOOK_RES_ERR, 1u);
    frl_wave_add(res + FRLOOK_RES_DISTINCT, won);
  }
  res[6] = (uint32_t)slot_words;
  res[7] = 0;
  if (!res[FRLOOK_RES_ERR]) {  // the plan's serial build (the host form of create) over the same keys: the same slots
    std::vector<uint32_t> again;
    res[7] = (uint32_t)frlook::build_serial(g, keys, again);
    if (memcmp(again.data(), slots, slot_words * 4)) return 2;
  }
  // k_frlook_count
  FrlPending pend = {FRLOOK_MISSING, 0};
  for (uint64_t e = 0; e < total && !res[FRLOOK_RES_ERR]; e++) {
    const size_t row = e / n, i = e - row * n;
    uint32_t j;
    const bool ok = frl_count_lane(g, keys, slots, f, row * stride + i, j);
    frl_count_tail(work.data(), idx, res, e, j, true, ok, pend);
  }
  frl_flush(work.data(), pend);
  // k_frlook_finish
  for (uint32_t j = 0; j < g.n_t; j++) frl_finish_lane(g, work.data(), j, m.data(), counts);
  memcpy(out.data() + 8 + slot_words + n_t + total, m.data(), n_t * 32);
  if (!write_file(argv[9], out)) return 2;
  return res[FRLOOK_RES_ERR] ? 3 : 0;
}
