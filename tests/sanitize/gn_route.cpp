// The GroupNorm route against its launcher, as text: for every "nimg hw C plan_nimg" of the command line (32 groups, one dense source; plan_nimg > 0: the
// images of one clip under deterministic batching, NrGnParams::plan_nimg) routes the
// GroupNorm (nr_gn_route), prints the route's status, kind, kernel count and scratch floats, and launches it (nr_launch_groupnorm) under
// tests/sanitize/hip_stub.cpp, whose NR_STUB_TRACE file lists the kernels that launch really enqueued behind a "# shape ..." line.  Built host-only
// like the engine's sources (launchers.h is HIP code); tests/test_launch_routes_host.py compares the two texts.
//   usage: gn_route <nimg> <hw> <C> <plan_nimg> [<nimg> <hw> <C> <plan_nimg> ...]
//          gn_route --c1-groups <nimg> <hw> <c0> <plan_nimg> <c1> <groups> [...]      a second dense source of c1 channels (0: none) and the group count;
//                                                                                     shape lines then read "shape nimg hw c0 plan_nimg c1 groups"
#include "launchers.h"
#include <cstdio>
#include <cstring>
#include <string>

extern "C" void nr_stub_note(const char* text);

int main(int argc, char** argv) {
  const bool wide = argc > 1 && !strcmp(argv[1], "--c1-groups");
  const int first = wide ? 2 : 1, per = wide ? 6 : 4;
  if (argc < first + per || (argc - first) % per != 0) { fprintf(stderr, "usage: gn_route [--c1-groups] <nimg> <hw> <C> <plan_nimg> [<c1> <groups>] ...\n"); return 1; }
  alignas(256) static char blk[4096];      // kernel launches are no-ops under the stub: one dummy block stands in for every tensor
  for (int i = first; i + per - 1 < argc; i += per) {
    const int nimg = atoi(argv[i]), hw = atoi(argv[i + 1]), C = atoi(argv[i + 2]);
    const int c1 = wide ? atoi(argv[i + 4]) : 0, groups = wide ? atoi(argv[i + 5]) : 32;
    NrGnParams p = nr_gn_params((const bf16*)blk, C, C, c1 ? (const bf16*)blk : nullptr, c1, c1, nimg, hw, groups, (const float*)blk, (const float*)blk, 1e-5f, 0,
                                (float*)blk, (bf16*)blk, C + c1);
    p.plan_nimg = atoi(argv[i + 3]);
    std::string shape = "shape " + std::to_string(nimg) + " " + std::to_string(hw) + " " + std::to_string(C) + " " + std::to_string(p.plan_nimg);
    if (wide) shape += " " + std::to_string(c1) + " " + std::to_string(groups);
    NrGnRoute r{};
    const int rc = nr_gn_route(&p, &r);
    printf("%s: status %d kind %d launches %d ws_floats %d\n", shape.c_str(), rc, r.kind, r.launches, r.ws_floats);
    nr_stub_note(shape.c_str());
    if (rc == 0 && nr_launch_groupnorm(&p, &r, nullptr) != 0) { fprintf(stderr, "FAIL: launch of %s\n", shape.c_str()); return 2; }
  }
  return 0;
}
