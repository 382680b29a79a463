// Stand-alone host program for tests/test_frhash2_host.py: a Poseidon2 handle of libmsm_frhash.so (MSM_FRHASH_POSEIDON2) run on the CPU -- the
// checks and the table of csrc/frhash_plan.h, and per permutation the very functions the kernels of csrc/frhash_kernels.h call, one lane after
// the other, each in its own slot of an array shaped like the workgroup's LDS and of the size the launch requests for this kind of handle (ONE
// copy of the state).  Built with g++ -DFQ_CHECK, so every limb and value bound of csrc/fq29.h is asserted along the way.
//   frhash2_harness permute <t> <R_F> <R_P> <flags> <tile> <n> <in> <out>                              in: rc, mu, n t states;  out: n t
//   frhash2_harness hash    <t> <R_F> <R_P> <flags> <tile> <rows> <len> <stride> <cap_at> <out_at> <in> <out>
//                                                                           in: rc, mu, capacity, (rows - 1) stride + len;  out: rows
//   frhash2_harness rules   <t>                          prints frh2_tidy_sums(t), frh2_bound(t), frh2_tidy_sbox(t) and FQ_HEADROOM
//   rc: R_F t + R_P scalars, mu: t.  flags: the call's (0 or MSM_FRHASH_MONT256).
//   exit status: 0 ok, 3 a value >= r among the elements read or the constants, 4 arguments the plan refuses, 2 a malformed command
// Compile with -DMSM_FIELD_NS=frh_<name> -DMSM_CURVE_CONSTANTS="fr_<name>_constants.h".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define MSM_CURVE_UNIT 1
#include MSM_CURVE_CONSTANTS
#include "fq29.h"
#include "frhash_kernels.h"
#include "frhash_plan.h"

using namespace MSM_FIELD_NS;
using namespace msm_frhash_plan;

static bool read_file(const char* path, std::vector<uint8_t>& out, size_t want) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  out.resize(want);
  const bool ok = want == 0 || fread(out.data(), 1, want, f) == want;
  fclose(f);
  return ok;
}
static bool write_file(const char* path, const uint32_t* words, size_t count) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(words, 4, count, f) == count;
  fclose(f);
  return ok;
}
static std::vector<uint32_t> words_of(const uint8_t* bytes, size_t count) {
  std::vector<uint32_t> w(count * 8);
  if (count) memcpy(w.data(), bytes, count * 32);
  return w;
}

struct Setup {
  uint32_t t, rf, rp, flags, tile;
  size_t n_rc, n_m;
  std::vector<uint32_t> table;
};
// 0, or the exit status
static int setup(char** argv, Setup& s) {
  s.t = (uint32_t)atoll(argv[2]), s.rf = (uint32_t)atoll(argv[3]), s.rp = (uint32_t)atoll(argv[4]), s.flags = (uint32_t)atoll(argv[5]), s.tile = (uint32_t)atoll(argv[6]);
  if ((s.flags & ~KNOWN_FLAGS) || !shape_ok(s.t, s.rf, s.rp, 5, MSM_FRHASH_POSEIDON2) || s.tile > FRHASH_THREADS) return 4;
  s.n_rc = constants_of(FRHASH_KIND_POSEIDON2, s.t, s.rf, s.rp), s.n_m = matrix_of(FRHASH_KIND_POSEIDON2, s.t);
  return 0;
}
static int make_table(const host_fr::Field& f, const uint8_t* in, Setup& s) {
  if (!all_below_r(f, in, s.n_rc + s.n_m)) return 3;
  plan_table(f, s.t, s.rf, s.rp, in, in + 32 * s.n_rc, s.table, FRHASH_KIND_POSEIDON2);
  if (s.table.size() != table_words(s.t, s.rf, s.rp, FRHASH_KIND_POSEIDON2)) return 2;
  return 0;
}
// a launch: every workgroup's lanes one after the other, through the kernel's own guard, on as much "LDS" as the launch asks for
template <typename Lane>
static bool launch(const FrhashArgs& g, Lane lane) {
  std::vector<uint32_t> lds(frhash_lds_bytes(g) / 4);
  bool ok = true;
  for (unsigned block = 0; block < blocks_of(g); block++)
    for (uint32_t thread = 0; thread < FRHASH_THREADS; thread++) {
      const uint32_t i = block * g.tile + thread;
      if (thread >= g.tile || i >= g.n) continue;
      ok &= lane(i, lds.data() + thread);
    }
  return ok;
}

static int run_permute(int argc, char** argv) {
  Setup s;
  if (argc != 10) return 2;
  if (int rc = setup(argv, s)) return rc;
  const size_t n = (size_t)atoll(argv[7]);
  if (!permute_args_ok(s.t, n, s.flags)) return 4;
  if (n > 4096) return 2;
  std::vector<uint8_t> in;
  if (!read_file(argv[8], in, (s.n_rc + s.n_m + n * s.t) * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  if (int rc = make_table(f, in.data(), s)) return rc;
  std::vector<uint32_t> state = words_of(in.data() + (s.n_rc + s.n_m) * 32, n * s.t);
  const FrhashArgs g = plan_args(s.t, s.rf, s.rp, n, s.flags, s.tile, FRHASH_KIND_POSEIDON2);
  const bool ok = launch(g, [&](uint32_t i, uint32_t* w) { return frh_permute_lane(g, i, state.data(), s.table.data(), state.data(), w); });  // (in place)
  return write_file(argv[9], state.data(), state.size()) ? (ok ? 0 : 3) : 2;
}

static int run_hash(int argc, char** argv) {
  Setup s;
  if (argc != 14) return 2;
  if (int rc = setup(argv, s)) return rc;
  const size_t rows = (size_t)atoll(argv[7]), len = (size_t)atoll(argv[8]), stride = (size_t)atoll(argv[9]);
  const uint32_t cap_at = (uint32_t)atoll(argv[10]), out_at = (uint32_t)atoll(argv[11]);
  if (!hash_args_ok(s.t, rows, len, stride, cap_at, out_at, s.flags)) return 4;
  const size_t span = (rows - 1) * stride + len;
  if (span > ((size_t)1 << 20)) return 2;
  std::vector<uint8_t> in;
  if (!read_file(argv[12], in, (s.n_rc + s.n_m + 1 + span) * 32)) return 2;
  const host_fr::Field f(FQ_P32);
  if (int rc = make_table(f, in.data(), s)) return rc;
  FrhashArgs g = plan_args(s.t, s.rf, s.rp, rows, s.flags, s.tile, FRHASH_KIND_POSEIDON2);
  g.len = (uint32_t)len, g.stride = (uint32_t)stride, g.capacity_at = cap_at, g.out_at = out_at;
  if (!plan_capacity(f, in.data() + (s.n_rc + s.n_m) * 32, g)) return 3;
  const std::vector<uint32_t> a = words_of(in.data() + (s.n_rc + s.n_m + 1) * 32, span);
  std::vector<uint32_t> out(rows * 8);
  const bool ok = launch(g, [&](uint32_t i, uint32_t* w) { return frh_hash_lane(g, i, a.data(), s.table.data(), out.data(), w); });
  return write_file(argv[13], out.data(), out.size()) ? (ok ? 0 : 3) : 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "permute")) return run_permute(argc, argv);
  if (!strcmp(argv[1], "hash")) return run_hash(argc, argv);
  if (!strcmp(argv[1], "rules") && argc == 3) {  // the kernel's tidy rules, for tools/bench_frhash.py's product count to be compared with
    const uint32_t t = (uint32_t)atoll(argv[2]);
    if (!poseidon2_width(t)) return 4;
    printf("%d %u %d %d\n", (int)frh2_tidy_sums(t), frh2_bound(t), (int)frh2_tidy_sbox(t), (int)FQ_HEADROOM);
    return 0;
  }
  return 2;
}
