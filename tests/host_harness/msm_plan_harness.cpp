// The launch planner of libmsm_hip.so (csrc/msm_plan.h) on the CPU: g++ -O2 -std=c++17 -I msm-webgpu_amd/csrc, no HIP.  Driven by
// tests/test_msm_plan_host.py and tests/test_gpu_plan_agrees.py.  Cases arrive on stdin, one per line: a verb and key=value tokens (a key left out
// keeps the default of its struct), one answer line each.
//   plan   the PlanInputs fields, cus (what num_cus() answers), null_ctx, the LaunchRequest fields -- scalars / indices / sums_dev: 0 null, 1 a dummy
//          pointer; align: the byte offset of the scalars' dummy from a 64-byte boundary --, whole: 1 = through whole_msm_request first
//          -> rc=<plan_launch's code> and, for rc = 0, every LaunchPlan field
//   group  the PlanInputs fields, n, batch -> group=<batch_group>
//   wide   curve, bits, n, wide_bits_choice -> top_max, fit, top_pos, pick (wide_top_max, wide_bits_fit, wide_top_pos, pick_wide_bits)
//   consts -> the limits the planner works within
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "msm_plan.h"

namespace {
size_t g_cus = 256;
inline size_t num_cus() { return g_cus; }

using Case = std::map<std::string, long long>;
long long get(const Case& c, const char* key, long long dflt) {
  const auto it = c.find(key);
  return it == c.end() ? dflt : it->second;
}

PlanInputs inputs_of(const Case& c) {
  PlanInputs in;
  in.curve = (int)get(c, "curve", in.curve);
  in.n_bases = (size_t)get(c, "n_bases", 0);
  in.precomputed = get(c, "precomputed", 0) != 0;
  in.wide_bits_choice = (int)get(c, "wide_bits_choice", 0);
  in.wide_bits = (int)get(c, "wide_bits", 0);
  in.endo = get(c, "endo", 0) != 0;
  in.n_identity = (size_t)get(c, "n_identity", 0);
  in.scalar_format = (uint32_t)get(c, "scalar_format", 0);
  in.window_bits = (int)get(c, "window_bits", 0);
  in.debug = get(c, "debug", 0) != 0;
  return in;
}

alignas(64) unsigned char g_dummy[128];  // never read: the planner looks at the pointers' values alone

void plan(const Case& c) {
  const PlanInputs in = inputs_of(c);
  g_cus = (size_t)get(c, "cus", 256);
  LaunchRequest r;
  r.scalars = get(c, "scalars", 1) ? g_dummy + get(c, "align", 0) : nullptr;
  r.n = (size_t)get(c, "n", 0);
  r.slot = (int)get(c, "slot", r.slot);
  r.nvec = (int)get(c, "nvec", r.nvec);
  r.sums_dev = get(c, "sums_dev", 0) ? g_dummy : nullptr;
  r.mode = (LaunchMode)get(c, "mode", r.mode);
  r.w_begin = (int)get(c, "w_begin", r.w_begin);
  r.w_end = (int)get(c, "w_end", r.w_end);
  r.wbits = (int)get(c, "wbits", r.wbits);
  r.v_begin = (int)get(c, "v_begin", r.v_begin);
  r.v_count = (int)get(c, "v_count", r.v_count);
  r.sparse = get(c, "sparse", 0) != 0;
  r.indices = get(c, "indices", 0) ? reinterpret_cast<const uint32_t*>(g_dummy + 64) : nullptr;
  r.base_off = (size_t)get(c, "base_off", 0);
  r.sync = get(c, "sync", 0) != 0;
  const PlanInputs* ctx = get(c, "null_ctx", 0) ? nullptr : &in;
  if (get(c, "whole", 0) && ctx) r = whole_msm_request(ctx, r);
  LaunchPlan p;
  const int rc = plan_launch(ctx, r, p);
  if (rc) {
    printf("rc=%d\n", rc);
    return;
  }
  printf("rc=0 n=%zu slot=%d nvec=%d sums_dev=%d mode=%d w_begin=%d w_end=%d wbits=%d v_begin=%d v_count=%d sparse=%d base_off=%zu sync=%d", p.n, p.slot, p.nvec,
         p.sums_dev != nullptr, (int)p.mode, p.w_begin, p.w_end, p.wbits, p.v_begin, p.v_count, (int)p.sparse, p.base_off, (int)p.sync);
  printf(" nb=%d nb_signed=%d nb_kernel=%d w_count_vec=%d wide_bits=%d pairs=%d half=%u ncoarse=%u w_count=%d nwin=%d combine_bits=%d whole=%d", p.nb, (int)p.nb_signed,
         p.nb_kernel(), p.w_count_vec, p.wide_bits, (int)p.pairs, p.half, p.ncoarse, p.w_count, p.nwin, p.combine_bits, (int)p.whole);
  printf(" n_sc=%zu n_entries=%zu full_windows=%d digits=%d planes=%d share_shape=%d list_path=%d tiles=%u tile_len=%u subtiles=%u chunks=%u chunk_len=%u stride=%zu",
         p.n_sc, p.n_entries, p.full_windows, (int)p.digits, (int)p.planes, (int)p.share_shape, (int)p.list_path, p.tiles, p.tile_len, p.subtiles, p.chunks, p.chunk_len,
         p.stride);
  printf(" mask=%d fine_hist=%d\n", (int)p.mask, (int)p.fine_hist);
}

void group(const Case& c) {
  const PlanInputs in = inputs_of(c);
  g_cus = (size_t)get(c, "cus", 256);
  printf("group=%zu\n", batch_group(&in, (size_t)get(c, "n", 0), (size_t)get(c, "batch", 0)));
}

void wide(const Case& c) {
  PlanInputs in;
  in.curve = (int)get(c, "curve", 0);
  in.wide_bits_choice = (int)get(c, "wide_bits_choice", 0);
  const int bits = (int)get(c, "bits", 16);
  printf("top_max=%u fit=%d top_pos=%d pick=%d\n", wide_top_max(in.curve, bits), (int)wide_bits_fit(in.curve, bits), wide_top_pos(bits),
         pick_wide_bits(&in, (size_t)get(c, "n", 0)));
}
}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string verb, tok;
    if (!(in >> verb)) continue;
    Case c;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) {
        fprintf(stderr, "bad token: %s\n", tok.c_str());
        return 2;
      }
      c[tok.substr(0, eq)] = std::stoll(tok.substr(eq + 1));
    }
    if (verb == "plan") plan(c);
    else if (verb == "group") group(c);
    else if (verb == "wide") wide(c);
    else if (verb == "consts")
      printf("MAXLW=%d BYTE_MAXLW=%d NWIN=%d MAX_TILES=%u MAX_POINTS=%zu NSLOT=%d SMVP_CHUNK_MIN=%d SMVP_CHUNK_MAX=%d SMVP_TARGET_LANES=%d LIST_SUB=%d target_lanes=%zu chunk_search=%d\n",
             MAXLW, BYTE_MAXLW, NWIN, MAX_TILES, MAX_POINTS, NSLOT, SMVP_CHUNK_MIN, SMVP_CHUNK_MAX, SMVP_TARGET_LANES, LIST_SUB, target_lanes(), (int)chunk_search());
    else {
      fprintf(stderr, "unknown verb: %s\n", verb.c_str());
      return 2;
    }
  }
  return 0;
}
