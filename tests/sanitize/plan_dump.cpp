// What the engine plans, as text: for every network of a schema file (the format planner_dryrun reads; tools/plan_schema.py writes it) and every
// plan shape / mode listed below it plans, runs ONE eager forward and prints each op description, the workspace and weight bytes and the export
// manifest.  Linked against tests/sanitize/hip_stub.cpp, whose NR_STUB_TRACE file adds every kernel launch, device allocation and uploaded
// weight.  tools/plan_equal.sh builds this driver against two trees of the engine and diffs both texts: the acceptance instrument of a host-side
// engine refactor.  Shapes of one network are planned one after another on ONE handle, so what an earlier plan left in the weight cache counts too.
//   usage: plan_dump <schema-file> [name,name,...]     (only these networks; the switches read once per process need a run of their own)
#include "../../include/neurons_amd.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

struct Net { nr_net_config cfg; std::vector<std::pair<std::string, std::vector<int64_t>>> tensors; };

#define CHECK(cond, msg) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, msg, nr_last_error()); exit(2); } } while (0)
#define OK(call) CHECK((call) == NR_OK, #call)

static void load_all(nr_net* h, const Net& n, unsigned seed) {      // the values planner_dryrun loads
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

struct Shape { int b, f, h, w, ctx; };
enum Mode { PLAIN, DET_BATCH, DEBUG_TAPS, CFG_PAIR, COND_FRAME0 };
struct Case { Shape s; Mode mode; };
static const char* mode_name[] = {"plain", "deterministic-batch", "debug-taps", "cfg-pair-identical", "condition-frames={0}"};

// rows of a leaf plan = b * f * h * w
static const std::map<std::string, std::vector<Case>> g_cases = {
    {"tiny_unet", {{{2, 8, 8, 8, 77}, PLAIN}, {{4, 16, 16, 8, 77}, PLAIN}, {{2, 8, 8, 8, 77}, DET_BATCH}, {{4, 16, 16, 8, 77}, DET_BATCH},
                   {{2, 8, 8, 8, 77}, DEBUG_TAPS}, {{2, 8, 8, 8, 77}, CFG_PAIR}}},
    {"tiny_ctrl", {{{2, 8, 8, 8, 77}, PLAIN}, {{8, 8, 8, 8, 77}, PLAIN}, {{2, 8, 8, 8, 77}, COND_FRAME0}}},
    {"tiny_ctrl_image", {{{2, 8, 8, 8, 77}, PLAIN}, {{2, 8, 8, 8, 77}, COND_FRAME0}}},
    // C = 320: 4608 / 128 / 9216 rows (the dry-run's), 4096 and 512 rows
    {"leaf_transformer", {{{1, 2, 48, 48, 77}, PLAIN}, {{1, 2, 8, 8, 77}, PLAIN}, {{2, 2, 48, 48, 77}, PLAIN}, {{1, 4, 32, 32, 77}, PLAIN}, {{1, 2, 16, 16, 77}, PLAIN},
                          {{2, 16, 16, 16, 77}, DET_BATCH}}},
    {"leaf_temporal", {{{1, 16, 16, 16, 0}, PLAIN}, {{1, 16, 8, 8, 0}, PLAIN}, {{2, 16, 16, 16, 0}, PLAIN}, {{1, 16, 4, 8, 0}, PLAIN}, {{4, 16, 16, 16, 0}, DET_BATCH}}},
    // C = 640: 256 / 2048 / 4096 rows and 16 frames
    {"leaf_transformer640", {{{2, 2, 8, 8, 77}, PLAIN}, {{2, 1, 32, 32, 77}, PLAIN}, {{2, 2, 32, 32, 77}, PLAIN}, {{1, 16, 8, 8, 77}, PLAIN}, {{1, 16, 16, 16, 77}, PLAIN}}},
    {"leaf_temporal640", {{{1, 16, 8, 8, 0}, PLAIN}, {{1, 8, 8, 8, 0}, PLAIN}, {{1, 16, 4, 4, 0}, PLAIN}, {{1, 16, 8, 16, 0}, PLAIN}, {{1, 16, 16, 16, 0}, PLAIN}}},
    // C = 1280: 2048 rows (and the 256 rows of the small-M kernel)
    {"leaf_transformer1280", {{{2, 1, 32, 32, 77}, PLAIN}, {{1, 16, 8, 16, 77}, PLAIN}, {{2, 2, 8, 8, 77}, PLAIN}}},
    {"leaf_temporal1280", {{{1, 16, 8, 16, 0}, PLAIN}, {{1, 16, 4, 4, 0}, PLAIN}}},
    {"tiny_sgm", {{{2, 1, 16, 16, 7}, PLAIN}}},
    {"tiny_vae_dec", {{{2, 1, 8, 8, 0}, PLAIN}}},
    {"tiny_vae_enc", {{{2, 1, 64, 64, 0}, PLAIN}}},
    {"tiny_clip", {{{2, 1, 1, 77, 0}, PLAIN}}},
};

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: plan_dump <schema-file> [name,name,...]\n"); return 1; }
  const std::string only = argc > 2 ? std::string(",") + argv[2] + "," : std::string();
  FILE* f = fopen(argv[1], "r");
  CHECK(f, "schema file");
  std::vector<std::pair<std::string, Net>> nets;      // in file order
  char line[4096];
  while (fgets(line, sizeof(line), f)) {
    if (line[0] == 'N') {
      std::vector<long> v;
      const std::string name = strtok(line + 2, " \n");
      while (char* tok = strtok(nullptr, " \n")) v.push_back(atol(tok));
      nets.emplace_back(name, Net{});
      Net& n = nets.back().second;
      std::memset(&n.cfg, 0, sizeof(n.cfg));
      CHECK(v.size() * sizeof(int32_t) == sizeof(nr_net_config), "config width");
      for (size_t i = 0; i < v.size(); ++i) reinterpret_cast<int32_t*>(&n.cfg)[i] = (int32_t)v[i];
    } else if (line[0] == 'T') {
      const std::string key = strtok(line + 2, " \n");
      const int nd = atoi(strtok(nullptr, " \n"));
      std::vector<int64_t> shape;
      for (int i = 0; i < nd; ++i) shape.push_back(atoll(strtok(nullptr, " \n")));
      nets.back().second.tensors.emplace_back(key, shape);
    }
  }
  fclose(f);
  const float ts[64] = {500.f, 500.f, 480.f, 480.f};
  std::vector<float> io((size_t)64 << 20);          // one host block standing in for every "device" I/O tensor
  float* sample = io.data();
  float* ctx = io.data() + (8 << 20);
  float* out = io.data() + (16 << 20);
  float* cond = io.data() + (24 << 20);
  float* mask = io.data() + (28 << 20);

  unsigned seed = 0;
  for (auto& nn : nets) {
    ++seed;
    const std::string& name = nn.first;
    const Net& n = nn.second;
    if (!only.empty() && only.find("," + name + ",") == std::string::npos) continue;
    CHECK(g_cases.count(name), ("no plan shapes listed for network " + name).c_str());
    nr_net* h = nullptr;
    OK(nr_net_create(&n.cfg, &h));
    load_all(h, n, seed);
    const int kind = n.cfg.kind;
    for (const Case& c : g_cases.at(name)) {
      const Shape& s = c.s;
      OK(nr_net_set_deterministic_batch(h, c.mode == DET_BATCH));
      OK(nr_net_set_debug(h, c.mode == DEBUG_TAPS));
      OK(nr_net_set_cfg_pair_identical(h, c.mode == CFG_PAIR));
      if (kind == NR_KIND_SPARSECTRL) {
        const int32_t frame0 = 0;
        OK(nr_sparsectrl_set_condition_frames(h, &frame0, c.mode == COND_FRAME0 ? 1 : -1));
      }
      printf("== %s plan batch=%d frames=%d h=%d w=%d ctx=%d mode=%s\n", name.c_str(), s.b, s.f, s.h, s.w, s.ctx, mode_name[c.mode]);
      OK(nr_net_plan(h, s.b, s.f, s.h, s.w, s.ctx));
      // one eager forward: the launches of the plan reach the stub's trace
      std::vector<std::vector<unsigned short>> resbuf;
      std::vector<void*> res;
      if (kind == NR_KIND_UNET3D || kind == NR_KIND_SPARSECTRL) {
        const int nres = nr_net_num_residuals(h);
        for (int i = 0; i <= nres; ++i) {
          int32_t C, hh, ww;
          OK(nr_net_residual_shape(h, i, &C, &hh, &ww));
          resbuf.emplace_back((size_t)s.b * s.f * hh * ww * C);
        }
        for (auto& b : resbuf) res.push_back(b.data());
        if (kind == NR_KIND_UNET3D) OK(nr_unet3d_forward(h, nullptr, sample, ts, ctx, s.ctx, (const void* const*)res.data(), res[nres], out));
        else OK(nr_sparsectrl_forward(h, nullptr, sample, ts, ctx, s.ctx, cond, mask, 1, 1.0f, res.data(), res[nres]));
      } else if (kind == NR_KIND_SGM_UNET) {
        OK(nr_sgm_unet_forward(h, nullptr, sample, 0.5f, ts, ctx, s.ctx, cond, out));
      } else if (kind == NR_KIND_VAE_DECODER) {
        OK(nr_vae_decode(h, nullptr, sample, 5.4f, 0.5f, 0.5f, 1, out));
      } else if (kind == NR_KIND_VAE_ENCODER) {
        OK(nr_vae_encode(h, nullptr, sample, 2.f, -1.f, out));
      } else if (kind == NR_KIND_CLIP_TEXT) {
        OK(nr_clip_text_forward(h, nullptr, reinterpret_cast<const int32_t*>(sample), out));
      } else {
        OK(nr_leaf_forward(h, nullptr, sample, s.ctx ? ctx : nullptr, s.ctx, out));
      }
      for (int i = 0; i < nr_net_num_ops(h); ++i) printf("op %d: %s\n", i, nr_net_op_desc(h, i));
      for (int i = 0; i < nr_net_num_taps(h); ++i) printf("tap %d: %s\n", i, nr_net_tap_name(h, i));
      printf("residuals: %d\n", (int)nr_net_num_residuals(h));
      printf("workspace_bytes: %lld\nweight_bytes: %lld\n", (long long)nr_net_workspace_bytes(h), (long long)nr_net_weight_bytes(h));
      int64_t arena = 0;
      const int64_t mlen = nr_net_export_manifest(h, nullptr, 0, &arena);
      CHECK(mlen > 0, "manifest size");
      std::vector<char> man((size_t)mlen);
      CHECK(nr_net_export_manifest(h, man.data(), mlen, &arena) == mlen, "manifest");
      printf("manifest (%lld bytes of arena):\n%.*s", (long long)arena, (int)mlen, man.data());
    }
    nr_net_destroy(h);
  }
  return 0;
}
