// Stand-alone driver of the weight-gradient plan and the ConvTranspose2d geometry (csrc/conv_plan.h) for
// tests/test_wgrad_plan_cpu.py: no HIP, no GPU. stdin, one request per line:
//   wgrad N H W C1 C2 Cout taps packed cin_real KERNEL splits slab FORM
//         (KERNEL: a name such as AUTO or HALO, or a number; slab: elements offered; FORM: conv, upT or firstbn)
//   upT fwd|dgrad N h w Cin C H2 W2 oy ox     (dense tensors: ldw = the GEMM's K, pitches = channels)
// stdout, one line per request, key=value pairs.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "conv_plan.h"

static int kernel_of(const std::string& t) {
  for (int i = 0; i < rdp_wgrad_kernel_count; ++i)
    if (t == rdp_wgrad_kernel_names[i].name) return rdp_wgrad_kernel_names[i].kernel;
  char* end = nullptr;
  const long v = strtol(t.c_str(), &end, 10);
  if (end == t.c_str() || *end) {
    fprintf(stderr, "unknown kernel '%s'\n", t.c_str());
    exit(2);
  }
  return (int)v;
}

static int bad(const std::string& line) {
  fprintf(stderr, "bad request: %s\n", line.c_str());
  return 2;
}

int main() {
  std::string line;
  long n = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "wgrad") {
      RdpWgradQuery q;
      std::string kern, form;
      if (!(in >> q.N >> q.H >> q.W >> q.C1 >> q.C2 >> q.Cout >> q.taps >> q.packed >> q.cin_real >> kern >> q.splits >>
            q.slab_elems >> form))
        return bad(line);
      q.kernel = kernel_of(kern);
      q.upT = form == "upT";
      q.first_bn = form == "firstbn";
      const RdpWgradPlan p = rdp_wgrad_plan_dense(q);
      const int Cin = q.packed ? 8 : q.C1 + q.C2;
      printf("status=%d kernel=%s bn=%d mr=%d tiles=%d splits=%d per=%d grid=%d block=%d slab=%ld G=%d g1=%d g2=%d "
             "vec=%d gen=%ld wave=%ld auto=%d\n",
             p.status, rdp_wgrad_kernel_name(p.kernel), p.BN, (int)p.multirow, p.tiles, p.splits, p.per_split, p.grid,
             p.block, p.slab_elems, p.reduce.G, p.reduce.grid1, p.reduce.grid2, p.reduce.vec,
             rdp_conv_wgrad_slab_elems(q.N, q.H, q.W, Cin, q.Cout, q.taps, q.packed, q.splits),
             rdp_conv_wgrad_halo_slab_elems(q.N, q.H, q.W, Cin, q.Cout),
             rdp_wgrad_auto_splits(q.N, q.H, q.W, Cin, q.Cout, q.taps, q.packed, 512));
    } else if (cmd == "upT") {
      std::string dir;
      int N, h, w, Cin, C;
      RdpUpT t;
      if (!(in >> dir >> N >> h >> w >> Cin >> C >> t.H2 >> t.W2 >> t.oy >> t.ox)) return bad(line);
      const RdpUpTGeo g = rdp_upT_geo_dense(dir == "fwd", N, h, w, Cin, C, t);
      printf("fits=%d bn=%d grid=%d tlc=%d\n", (int)g.fits, g.BN, g.grid, g.tlc);
    } else {
      fprintf(stderr, "unknown command '%s'\n", cmd.c_str());
      return 2;
    }
    ++n;
  }
  fprintf(stderr, "%ld requests\n", n);
  return 0;
}
