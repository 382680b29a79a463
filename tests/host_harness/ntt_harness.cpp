// Stand-alone host program for tests/test_ntt_host.py: the scalar-field NTT of libmsm_fr.so run on the CPU -- the plan and the tables of
// csrc/ntt_plan.h, and per element the very functions a lane of k_ntt_pass runs (csrc/ntt_kernels.h: ntt_pass_load / _level / _store), one
// "workgroup" after the other.  Built with g++ -DFQ_CHECK, so every limb and value bound of csrc/fq29.h is asserted along the way.
//   ntt_harness <log_n> <pass_bits> <batch> <flags> <in> <out>
//   in:  omega[32]  has_pre[1] pre[32]  has_post[1] post[32]  data[batch * 2^log_n * 32];   out: the transformed data.   flags: 1 = scale by 1 / n
//   exit status: 0 ok, 3 a value >= r among the inputs, 2 bad arguments
// Compile with -DMSM_FIELD_NS=fr_<name> -DMSM_CURVE_CONSTANTS="fr_<name>_constants.h".
#include <cstdio>
#include <cstdlib>
#include <vector>

#define MSM_CURVE_UNIT 1
#include MSM_CURVE_CONSTANTS
#include "fq29.h"
#include "ntt_kernels.h"
#include "ntt_plan.h"

using namespace MSM_FIELD_NS;

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int log_n = atoi(argv[1]), cap = atoi(argv[2]), flags = atoi(argv[4]);
  const size_t batch = (size_t)atoll(argv[3]);
  if (log_n < 0 || log_n > 20 || cap < 1 || cap > NTT_PASS_BITS || batch < 1) return 2;
  const size_t n = (size_t)1 << log_n, words = batch * n * 8;
  FILE* fi = fopen(argv[5], "rb");
  if (!fi) return 2;
  uint8_t head[98];
  std::vector<uint32_t> data(words), scratch(words);
  if (fread(head, 1, 98, fi) != 98 || fread(data.data(), 4, words, fi) != words) return 2;
  fclose(fi);
  const uint8_t *omega = head, *pre = head[32] ? head + 33 : nullptr, *post = head[65] ? head + 66 : nullptr;
  const host_fr::Field f(FQ_P32);
  if (!host_fr::is_primitive_root(f, omega, log_n)) return 2;

  const std::vector<uint32_t> dig = msm_fr::plan_digits(log_n, cap);
  std::vector<NttPass> passes = msm_fr::plan_passes(log_n, dig);
  NttTables t = {};
  std::vector<uint32_t> bt;
  if (log_n > 0) bt = msm_fr::build_butterfly_table(f, omega, log_n, (int)passes[0].tw_log);
  t.bt = bt.data();
  msm_fr::HostTable tw, tpre, tpost;
  if (passes.size() > 1) tw = msm_fr::build_power_table(f, omega, log_n, 0);
  const int inv = (flags & 1) && log_n > 0 ? log_n : 0;
  if (pre) tpre = msm_fr::build_power_table(f, pre, log_n, 0);
  if (post || inv) tpost = msm_fr::build_power_table(f, post, log_n, inv);
  t.tw_lo = tw.lo.data(), t.tw_hi = tw.hi.data(), t.pre_lo = tpre.lo.data(), t.pre_hi = tpre.hi.data(), t.post_lo = tpost.lo.data(), t.post_hi = tpost.hi.data();
  for (NttPass& p : passes) {
    p.tw_mode = tw.mode, p.tw_lo_bits = tw.lo_bits;
    p.pre_mode = p.first ? tpre.mode : 0, p.pre_lo_bits = tpre.lo_bits;
    p.post_mode = p.last ? tpost.mode : 0, p.post_lo_bits = tpost.lo_bits;
  }
  bool ok = true;
  std::vector<fq> tile((size_t)1 << (NTT_PASS_BITS + NTT_COL_BITS));
  const size_t k = passes.size();
  for (size_t q = 0; q < k; q++) {
    const NttPass& p = passes[q];
    const uint32_t* src = (k > 1 && q == k - 1) ? scratch.data() : data.data();
    uint32_t* dst = (k > 1 && q == k - 2) ? scratch.data() : data.data();
    const uint32_t elems = 1u << (p.b + p.log_c);
    const size_t blocks = batch << (p.log_n - p.b - p.log_c);
    for (size_t blk = 0; blk < blocks; blk++) {
      const NttBlock kb = ntt_block(p, (uint32_t)blk);
      for (uint32_t e = 0; e < elems; e++) ok &= ntt_pass_load(p, t, kb, e, src, tile.data());
      for (uint32_t s = 0; s < p.b; s++)
        for (uint32_t x = 0; x < (elems >> 1); x++) ntt_pass_level(p, t, s, x, tile.data());
      for (uint32_t e = 0; e < elems; e++) ntt_pass_store(p, t, kb, e, tile.data(), dst);
    }
  }
  FILE* fo = fopen(argv[6], "wb");
  if (!fo || fwrite(data.data(), 4, words, fo) != words) return 2;
  fclose(fo);
  return ok ? 0 : 3;
}
