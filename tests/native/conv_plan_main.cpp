// Stand-alone driver of the conv plan (csrc/conv_plan.h) for tests/test_conv_plan_cpu.py: no HIP, no GPU.
// stdin, one request per line:
//   plan N H W C1 C2 Cout taps packed KERNEL stats eval split ws pool up bn wfrag bnin
//        (KERNEL: a name such as AUTO or PP256, or a number; ws: workspace elements offered, -1 = conv_ws_elems)
//   ws N H W C1 C2 Cout taps packed KERNEL
// stdout, one line per request, key=value pairs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "conv_plan.h"

static int kernel_of(const std::string& t) {
  for (int i = 0; i < rdp_conv_kernel_count; ++i)
    if (t == rdp_conv_kernel_names[i].name) return rdp_conv_kernel_names[i].kernel;
  char* end = nullptr;
  const long v = strtol(t.c_str(), &end, 10);
  if (end == t.c_str() || *end) {
    fprintf(stderr, "unknown kernel '%s'\n", t.c_str());
    exit(2);
  }
  return (int)v;
}

int main() {
  std::string line;
  long n = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, kern;
    if (!(in >> cmd)) continue;
    RdpConvQuery q;
    int stats = 0, eval = 0, pool = 0, up = 0, bn = 0, wfrag = 0, bnin = 0;
    long ws = 0;
    if (!(in >> q.N >> q.H >> q.W >> q.C1 >> q.C2 >> q.Cout >> q.taps >> q.packed >> kern)) {
      fprintf(stderr, "bad request: %s\n", line.c_str());
      return 2;
    }
    q.kernel = kernel_of(kern);
    const long need = rdp_conv_ws_elems(q.N, q.H, q.W, q.C1, q.C2, q.Cout, q.taps, q.packed, q.kernel);
    if (cmd == "ws") {
      printf("ws=%ld\n", need);
    } else if (cmd == "plan") {
      if (!(in >> stats >> eval >> q.split >> ws >> pool >> up >> bn >> wfrag >> bnin)) {
        fprintf(stderr, "bad request: %s\n", line.c_str());
        return 2;
      }
      q.stats = stats; q.eval = eval; q.pool = pool; q.up = up; q.bn = bn; q.wfrag = wfrag; q.bnin = bnin;
      q.ws_elems = ws < 0 ? need : ws;
      const RdpConvPlan p = rdp_conv_plan_dense(q);
      static const char* const forms[] = {"PLAIN", "POOL", "BNRED", "BNIN", "HEAD"};
      printf("kernel=%s form=%s code=%d bm=%d bn=%d waves=%d ksplit=%d mode=%d launches=%d grid=%d rgrid=%d rows=%d ws=%ld "
             "pool=%d up=%d bnrows=%d bound=%d need=%ld\n",
             rdp_conv_kernel_name(p.kernel), p.kernel == RDP_CONV_RING ? forms[p.ring_form] : "-", p.kernel, p.BM, p.BN,
             p.waves, p.ksplit, p.rowband_mode, p.launches, p.grid,
             p.rgrid, p.stats_rows, p.ws_elems, (int)p.pool_fused, (int)p.up_fused, p.bn_rows,
             rdp_conv_stats_rows((long)q.N * q.H * q.W, q.Cout, q.kernel), need);
    } else {
      fprintf(stderr, "unknown command '%s'\n", cmd.c_str());
      return 2;
    }
    ++n;
  }
  fprintf(stderr, "%ld requests\n", n);
  return 0;
}
