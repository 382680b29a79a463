// Stand-alone host program for tests/test_frgate_host.py: a call of libmsm_frgate.so run on the CPU -- the checks, offsets and term records of
// csrc/frgate_plan.h, and per element the very function the kernel of csrc/frgate_kernels.h calls, one lane after the other.  Built with
// g++ -DFQ_CHECK, so every limb and value bound of csrc/fq29.h is asserted along the way.
//   frgate_harness apply <n> <batch> <stride> <step> <scale_len> <flags> <terms> <in> <out>
//       in: terms[terms x 100] a[span] scale[scale_len] out[n];   out: out[n]
//       span = (batch - 1) stride + n; scale_len 0: no scale; a term is an msm_frgate_term; out is what the call finds in its output
//   frgate_harness offset <rot> <step> <n>        prints the element offset of a rotation
//   exit status: 0 ok, 3 a value >= r among the elements read, 4 arguments the plan refuses, 2 a malformed command
// Compile with -DMSM_FIELD_NS=frg_<name> -DMSM_CURVE_CONSTANTS="fr_<name>_constants.h".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define MSM_CURVE_UNIT 1
#include MSM_CURVE_CONSTANTS
#include "fq29.h"
#include "frgate_kernels.h"
#include "frgate_plan.h"

using namespace MSM_FIELD_NS;

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

static int run_apply(int argc, char** argv) {
  if (argc != 11) return 2;
  const size_t n = (size_t)atoll(argv[2]), batch = (size_t)atoll(argv[3]), stride = (size_t)atoll(argv[4]), step = (size_t)atoll(argv[5]);
  const size_t scale_len = (size_t)atoll(argv[6]);
  const uint32_t flags = (uint32_t)atoll(argv[7]);
  const size_t num_terms = (size_t)atoll(argv[8]);
  if (n < 1 || batch < 1 || stride < n || num_terms > 1024 || n > ((size_t)1 << 20) || batch * stride > ((size_t)1 << 22) || scale_len > n) return 2;
  const size_t span = (batch - 1) * stride + n;
  std::vector<uint8_t> in;
  if (!read_file(argv[9], in, num_terms * sizeof(msm_frgate_term) + (span + scale_len + n) * 32)) return 2;
  std::vector<msm_frgate_term> terms(num_terms);
  if (num_terms) memcpy(terms.data(), in.data(), num_terms * sizeof(msm_frgate_term));
  const bool has_scale = scale_len != 0;
  const host_fr::Field f(FQ_P32);
  if (!msm_frgate::args_ok(f, n, batch, stride, terms.data(), num_terms, step, has_scale, scale_len, flags)) return 4;
  std::vector<uint32_t> words;
  const FrgateArgs g = msm_frgate::plan_apply(f, n, stride, terms.data(), num_terms, step, has_scale, scale_len, flags, words);
  const uint8_t* data = in.data() + num_terms * sizeof(msm_frgate_term);
  const std::vector<uint32_t> a = words_of(data, span), scale = words_of(data + span * 32, scale_len);
  std::vector<uint32_t> out = words_of(data + (span + scale_len) * 32, n);
  bool ok = true;
  const size_t blocks = (n + FRGATE_THREADS - 1) / FRGATE_THREADS;
  for (size_t i = 0; i < blocks * FRGATE_THREADS; i++)  // (the kernel's own guard)
    if (i < g.n) ok &= frg_lane(g, (uint32_t)i, a.data(), words.data(), has_scale ? scale.data() : nullptr, out.data());
  return write_file(argv[10], out.data(), out.size()) ? (ok ? 0 : 3) : 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "apply")) return run_apply(argc, argv);
  if (!strcmp(argv[1], "offset") && argc == 5) {
    printf("%u\n", msm_frgate::offset_of((int32_t)atoll(argv[2]), (size_t)atoll(argv[3]), (size_t)atoll(argv[4])));
    return 0;
  }
  return 2;
}
