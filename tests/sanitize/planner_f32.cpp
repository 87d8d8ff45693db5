// Sanitizer dry-run of the planner at 32 frames (BASELINE config 5) on the C = 640 / 1280 temporal leaves: the host side of the 32-frame form of the temporal
// attention head kernel (tattnw.hip) -- the routing rule, the launch descriptions, the epilogue table cached PER FRAME COUNT beside the shared weight stream,
// the 16 -> 32 -> 16 -> ineligible re-plans and what a re-plan needs after nr_net_release_host_weights.  Linked like planner_dryrun.cpp: the engine compiled
// host-only with -fsanitize=address,undefined against hip_stub.cpp (device memory = host heap, launches are no-ops); tests/test_tattn_head_f32_planner_host.py.
//   usage: planner_f32 <schema-file>      schema lines as for planner_dryrun; nets "leaf_temporal640_pe32", "leaf_temporal1280_pe32" (motion_pe_max_len = 32)
#include "../../include/neurons_amd.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

extern "C" long nr_stub_live_allocs(void);
extern "C" long nr_stub_live_graphs(void);

struct Net { nr_net_config cfg; std::vector<std::pair<std::string, std::vector<int64_t>>> tensors; };

#define CHECK(cond, msg) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, msg, nr_last_error()); exit(2); } } while (0)
#define OK(call) CHECK((call) == NR_OK, #call)

static void load_all(nr_net* h, const Net& n, unsigned seed) {
  for (auto& t : n.tensors) {
    int64_t numel = 1;
    for (auto d : t.second) numel *= d;
    std::vector<float> data((size_t)numel);
    unsigned s = seed * 2654435761u + (unsigned)std::hash<std::string>()(t.first);
    const bool vec = t.second.size() == 1;
    for (auto& v : data) { s = s * 1664525u + 1013904223u; const float u = ((s >> 8) & 0xffff) / 65536.0f - 0.5f; v = vec ? (t.first.find("weight") != std::string::npos ? 1.0f + 0.1f * u : 0.05f * u) : 0.1f * u; }
    OK(nr_net_load_tensor(h, t.first.c_str(), data.data(), t.second.data(), (int32_t)t.second.size()));
  }
}

struct Plan { int heads = 0, cores = 0, qkv = 0; };
// counts of the current plan: "tattn_head M=<rows> C=<C> F=<frames>" launches, temporal attention cores, GEMMs with N = 3 C, K = C (a q|k|v projection)
static Plan count(nr_net* h, int rows, int C, int frames) {
  char want[96], nk[64];
  snprintf(want, sizeof(want), "tattn_head M=%d C=%d F=%d ", rows, C, frames);
  snprintf(nk, sizeof(nk), "N=%d K=%d", 3 * C, C);
  Plan p;
  for (int i = 0; i < nr_net_num_ops(h); ++i) {
    const char* d = nr_net_op_desc(h, i);
    if (strstr(d, "tattn_head")) { CHECK(strncmp(d, want, strlen(want)) == 0, d); ++p.heads; }
    p.cores += strstr(d, "attention mode=2") != nullptr;
    p.qkv += strstr(d, nk) != nullptr;
  }
  return p;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: planner_f32 <schema-file>\n"); return 1; }
  FILE* f = fopen(argv[1], "r");
  CHECK(f, "schema file");
  std::map<std::string, Net> nets;
  char line[4096], name[256];
  std::string cur;
  while (fgets(line, sizeof(line), f)) {
    if (line[0] == 'N') {
      std::vector<long> v;
      char* tok = strtok(line + 2, " \n");
      strncpy(name, tok, sizeof(name) - 1);
      name[sizeof(name) - 1] = 0;
      while ((tok = strtok(nullptr, " \n"))) v.push_back(atol(tok));
      cur = name;
      Net& n = nets[cur];
      std::memset(&n.cfg, 0, sizeof(n.cfg));
      int32_t* ci = reinterpret_cast<int32_t*>(&n.cfg);
      CHECK(v.size() * sizeof(int32_t) == sizeof(nr_net_config), "config width");
      for (size_t i = 0; i < v.size(); ++i) ci[i] = (int32_t)v[i];
    } else if (line[0] == 'T') {
      char* tok = strtok(line + 2, " \n");
      std::string key = tok;
      const int nd = atoi(strtok(nullptr, " \n"));
      std::vector<int64_t> shape;
      for (int i = 0; i < nd; ++i) shape.push_back(atoll(strtok(nullptr, " \n")));
      nets[cur].tensors.emplace_back(key, shape);
    }
  }
  fclose(f);
  std::vector<float> io((size_t)16 << 20);          // one host block standing in for the "device" input and output (<= 1280 x 32 x 8 x 8 floats each)
  float* sample = io.data();
  float* out = io.data() + (8 << 20);
  const long long table16 = 8LL * 16384, table32 = 2 * table16;      // C = 640: 8 heads x one 16-KiB part per 16 frames

  // ---------------- C = 640, pe max len 32: 16 -> 32 -> 16 -> 24 (not eligible) -> 32 on ONE handle ----------------
  {
    const Net& n = nets.at("leaf_temporal640_pe32");
    CHECK(n.cfg.motion_pe_max_len == 32 && n.cfg.motion_num_attention_blocks == 2, "schema: pe max len 32, two attention blocks");
    nr_net* h = nullptr;
    OK(nr_net_create(&n.cfg, &h));
    load_all(h, n, 21);
    // two clips of 16 frames = the 2048 rows of one clip of 32: every other layer of the module picks the same kernel (and the same converted weights)
    // in both plans, so the difference between the two is the temporal attention's alone
    OK(nr_net_plan(h, 2, 16, 8, 8, 0));
    OK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out));
    Plan p = count(h, 2048, 640, 16);
    CHECK(p.heads == 2 && p.cores == 0 && p.qkv == 0, "F = 16: one tattn_head launch per attention block, nothing else");
    const long long bytes16 = nr_net_weight_bytes(h);
    const long live16 = nr_stub_live_allocs();

    OK(nr_net_plan(h, 1, 32, 8, 8, 0));
    OK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out));
    p = count(h, 2048, 640, 32);
    CHECK(p.heads == 2 && p.cores == 0 && p.qkv == 0, "F = 32: one tattn_head ... F=32 launch per attention block, no q|k|v GEMM, no attention core");
    const long long bytes32 = nr_net_weight_bytes(h);
    printf("C = 640: weight bytes at 16 frames %lld, after the re-plan at 32 frames %lld (+%lld), device buffers %ld -> %ld\n", bytes16, bytes32, bytes32 - bytes16, live16, nr_stub_live_allocs());
    // the weight stream does not depend on F and is reused; each block gets a 32-position table BESIDE its 16-position one
    CHECK(bytes32 - bytes16 == 2 * table32, "re-plan 16 -> 32 must add exactly one two-part epilogue table per block");
    CHECK(nr_stub_live_allocs() == live16 + 2, "re-plan 16 -> 32: two new device buffers (the tables), nothing else");

    OK(nr_net_plan(h, 2, 16, 8, 8, 0));
    OK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out));
    p = count(h, 2048, 640, 16);
    CHECK(p.heads == 2 && p.cores == 0, "back at 16 frames");
    CHECK(nr_net_weight_bytes(h) == bytes32 && nr_stub_live_allocs() == live16 + 2, "both tables stay cached: nothing rebuilt, nothing leaked");

    OK(nr_net_plan(h, 2, 32, 16, 16, 0));                             // another 32-frame shape (other layers convert more weights at this row count)
    OK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out));
    p = count(h, 2 * 32 * 256, 640, 32);
    CHECK(p.heads == 2 && p.cores == 0, "a larger 32-frame shape (16 384 rows) runs the head kernel as well");

    OK(nr_net_plan(h, 1, 24, 8, 8, 0));                               // 24 frames: q|k|v GEMM + attention core (needs the folded matrix again)
    OK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out));
    p = count(h, 0, 640, 24);
    CHECK(p.heads == 0 && p.cores == 2 && p.qkv == 2, "F = 24 is not eligible for the head kernel");
    OK(nr_net_plan(h, 1, 32, 8, 8, 0));
    OK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out));
    p = count(h, 2048, 640, 32);
    CHECK(p.heads == 2 && p.cores == 0, "and back at 32 frames");
    CHECK(nr_net_plan(h, 1, 33, 8, 8, 0) == NR_ERR_ARG, "video_length beyond temporal_position_encoding_max_len");
    CHECK(nr_net_plan(h, 1, 32, 2, 6, 0) == NR_OK && count(h, 0, 640, 32).heads == 0 && count(h, 0, 640, 32).cores == 2, "hw = 12 is not a multiple of 8: three-launch sequence");

    // a reloaded to_q drops the stream and BOTH tables of its block; the next 32-frame plan rebuilds the stream and the 32-position table only
    OK(nr_net_plan(h, 1, 32, 8, 8, 0));
    const long long before_reload = nr_net_weight_bytes(h);
    for (auto& t : n.tensors)
      if (t.first.find("attention_blocks.0.to_q.weight") != std::string::npos) {
        int64_t numel = 1;
        for (auto d : t.second) numel *= d;
        std::vector<float> data((size_t)numel, 0.02f);
        OK(nr_net_load_tensor(h, t.first.c_str(), data.data(), t.second.data(), (int32_t)t.second.size()));
      }
    CHECK(nr_net_weight_bytes(h) <= before_reload - table16 - table32, "a reloaded to_q must drop the 16- and the 32-position table built from it");
    CHECK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out) == NR_ERR_STATE, "forward after a reload must ask for a new plan");
    OK(nr_net_plan(h, 1, 32, 8, 8, 0));
    OK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out));
    p = count(h, 2048, 640, 32);
    CHECK(p.heads == 2, "re-plan after the reload");
    nr_net_destroy(h);
  }
  // ---------------- re-plan from an eligible shape to an ineligible one AFTER nr_net_release_host_weights: the same answer at 32 frames as at 16 ----------------
  {
    const Net& n = nets.at("leaf_temporal640_pe32");
    nr_status st[2];
    const int eligible[2] = {16, 32}, ineligible[2] = {8, 24};
    for (int k = 0; k < 2; ++k) {
      nr_net* h = nullptr;
      OK(nr_net_create(&n.cfg, &h));
      load_all(h, n, 22);
      OK(nr_net_plan(h, 1, eligible[k], 8, 8, 0));
      OK(nr_net_release_host_weights(h));
      OK(nr_net_plan(h, 1, eligible[k], 8, 8, 0));                   // the same shape again: every conversion is cached
      OK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out));
      st[k] = nr_net_plan(h, 1, ineligible[k], 8, 8, 0);             // needs the folded [3C][C] matrix the stream pack dropped: host data is gone
      CHECK(st[k] == NR_OK || st[k] == NR_ERR_STATE || st[k] == NR_ERR_MISSING_WEIGHT, "a specific status, not a crash");
      printf("re-plan %d -> %d frames after nr_net_release_host_weights: status %d (%s)\n", eligible[k], ineligible[k], (int)st[k], st[k] == NR_OK ? "ok" : nr_last_error());
      if (st[k] != NR_OK) {                                           // the handle stays usable at the shape it has conversions for
        OK(nr_net_plan(h, 1, eligible[k], 8, 8, 0));
        OK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out));
      }
      nr_net_destroy(h);
    }
    CHECK(st[0] == st[1], "32 frames must behave as 16 frames do");
  }
  // ---------------- C = 1280: the 2048-row floor holds at 32 frames ----------------
  {
    const Net& n = nets.at("leaf_temporal1280_pe32");
    nr_net* h = nullptr;
    OK(nr_net_create(&n.cfg, &h));
    load_all(h, n, 23);
    OK(nr_net_plan(h, 1, 32, 8, 8, 0));                               // 2048 rows
    OK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out));
    Plan p = count(h, 2048, 1280, 32);
    CHECK(p.heads == 2 && p.cores == 0 && p.qkv == 0, "C = 1280, F = 32 at 2048 rows: the head kernel");
    const long long b32 = nr_net_weight_bytes(h);
    OK(nr_net_plan(h, 1, 32, 4, 4, 0));                               // 512 rows: below the floor
    OK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out));
    p = count(h, 0, 1280, 32);
    CHECK(p.heads == 0 && p.cores == 2, "C = 1280, F = 32 at 512 rows: three-launch sequence");
    OK(nr_net_plan(h, 2, 16, 8, 8, 0));                               // 2048 rows at 16 frames: its own (one-part) table
    OK(nr_leaf_forward(h, nullptr, sample, nullptr, 0, out));
    p = count(h, 2048, 1280, 16);
    CHECK(p.heads == 2 && p.cores == 0, "C = 1280, F = 16 at 2048 rows");
    CHECK(nr_net_weight_bytes(h) >= b32 + 2 * 8LL * 32768, "a 16-position table per block beside the 32-position one");
    nr_net_destroy(h);
  }
  CHECK(nr_stub_live_graphs() == 0, "graph executables leaked");
  printf("planner f32 dry-run OK\n");
  return 0;
}
