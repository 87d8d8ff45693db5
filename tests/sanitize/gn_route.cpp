// The GroupNorm route against its launcher, as text: for every "nimg hw C plan_nimg" of the command line (32 groups, one dense source; plan_nimg > 0: the
// images of one clip under deterministic batching, NrGnParams::plan_nimg) routes the
// GroupNorm (nr_gn_route), prints the route's status, kind, kernel count and scratch floats, and launches it (nr_launch_groupnorm) under
// tests/sanitize/hip_stub.cpp, whose NR_STUB_TRACE file lists the kernels that launch really enqueued behind a "# shape ..." line.  Built host-only
// like the engine's sources (launchers.h is HIP code); tests/test_launch_routes_host.py compares the two texts.
//   usage: gn_route <nimg> <hw> <C> <plan_nimg> [<nimg> <hw> <C> <plan_nimg> ...]
#include "launchers.h"
#include <cstdio>
#include <string>

extern "C" void nr_stub_note(const char* text);

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 1) % 4 != 0) { fprintf(stderr, "usage: gn_route <nimg> <hw> <C> <plan_nimg> ...\n"); return 1; }
  alignas(256) static char blk[4096];      // kernel launches are no-ops under the stub: one dummy block stands in for every tensor
  for (int i = 1; i + 3 < argc; i += 4) {
    const int nimg = atoi(argv[i]), hw = atoi(argv[i + 1]), C = atoi(argv[i + 2]);
    NrGnParams p = nr_gn_params((const bf16*)blk, C, C, nullptr, 0, 0, nimg, hw, 32, (const float*)blk, (const float*)blk, 1e-5f, 0, (float*)blk, (bf16*)blk, C);
    p.plan_nimg = atoi(argv[i + 3]);
    const std::string shape = "shape " + std::to_string(nimg) + " " + std::to_string(hw) + " " + std::to_string(C) + " " + std::to_string(p.plan_nimg);
    NrGnRoute r{};
    const int rc = nr_gn_route(&p, &r);
    printf("%s: status %d kind %d launches %d ws_floats %d\n", shape.c_str(), rc, r.kind, r.launches, r.ws_floats);
    nr_stub_note(shape.c_str());
    if (rc == 0 && nr_launch_groupnorm(&p, &r, nullptr) != 0) { fprintf(stderr, "FAIL: launch of %s\n", shape.c_str()); return 2; }
  }
  return 0;
}
