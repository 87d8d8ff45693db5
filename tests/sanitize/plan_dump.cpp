// What the engine plans, as text: for every network of a schema file (the format planner_dryrun reads; tools/plan_schema.py writes it) and every
// plan shape / mode listed below it plans, runs ONE eager forward and prints each op description, the workspace and weight bytes and the export
// manifest.  Linked against tests/sanitize/hip_stub.cpp, whose NR_STUB_TRACE file adds every kernel launch, device allocation and uploaded
// weight.  tools/plan_equal.sh builds this driver against two trees of the engine and diffs both texts: the acceptance instrument of a host-side
// engine refactor.  Shapes of one network are planned one after another on ONE handle, so what an earlier plan left in the weight cache counts too.
//   usage: plan_dump <schema-file> [name,name,...]     (only these networks; the switches read once per process need a run of their own)
//          plan_dump --ops <shapes-file>               every GEMM / conv op hook (nr_op_gemm, _gemm2, _ln_gemm, _gemm_ex, _conv3x3, _conv3x3_tap_inner) at the shapes
//                                                      of the file (tests/sanitize/op_route_shapes.txt), once per gemm8p mode 0 / 1 / 2 x NR_SMALLM unset / 0 / 2: which
//                                                      kernel each hook launches, in the trace
//          plan_dump --decide-once <schema-file>       the C = 1280 transformer leaf at 1024 rows planned under gemm8p mode 2 and replayed (graph off) before and after
//                                                      nr_g8p_set_mode(1) + NR_IGEMM_FORCE: a plan launches what it was planned with (tests/test_gemm_route_host.py)
//          plan_dump --ff-waves <schema-file>          the C = 320 temporal and transformer leaves at 4096 rows (ff_fused, tattn_fused / xattn_fused, GroupNorm, attention)
//                                                      planned under 8 FeedForward waves and replayed (graph off) before and after nr_ff_set_waves(4), then planned
//                                                      afresh under 4: the wave count is the plan's (tests/test_launch_routes_host.py)
//          plan_dump --force-sweep                     the tiled igemm under every NR_IGEMM_FORCE string of bm {64, 128, 256} x bn {32, 64, 128, 160} x stages 2 .. 8 x
//                                                      waves {-1, 4, 8, 41}: per string one small call of each request kind (Linear, GEGLU Linear, LayerNorm-folded
//                                                      Linear plain and GEGLU, 3x3 conv, two-source 3x3 conv, phase-form upsample conv) through its op hook, with
//                                                      the route's tiled plan as a note in front of the launch lines (tests/test_igemm_table_host.py)
#include "../../include/neurons_amd.h"
#include "launchers.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

extern "C" void nr_stub_note(const char* text);

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
    // the noisy sample not zeroed (conv_in(sample) + the embedding), a motion module in the mid block, 17 residual adds (one launch each)
    {"tiny_ctrl_noisy", {{{2, 8, 8, 8, 77}, PLAIN}, {{4, 8, 8, 8, 77}, PLAIN}}},
    {"tiny_ctrl_image_noisy", {{{2, 8, 8, 8, 77}, PLAIN}}},
    {"tiny_unet_midmotion", {{{2, 8, 8, 8, 77}, PLAIN}}},
    {"tiny_unet_lpb3", {{{2, 8, 8, 8, 77}, PLAIN}}},
    // C = 320: 4608 / 128 / 9216 rows (the dry-run's), 4096 and 512 rows
    {"leaf_transformer", {{{1, 2, 48, 48, 77}, PLAIN}, {{1, 2, 8, 8, 77}, PLAIN}, {{2, 2, 48, 48, 77}, PLAIN}, {{1, 4, 32, 32, 77}, PLAIN}, {{1, 2, 16, 16, 77}, PLAIN},
                          {{2, 16, 16, 16, 77}, DET_BATCH}}},
    {"leaf_temporal", {{{1, 16, 16, 16, 0}, PLAIN}, {{1, 16, 8, 8, 0}, PLAIN}, {{2, 16, 16, 16, 0}, PLAIN}, {{1, 16, 4, 8, 0}, PLAIN}, {{4, 16, 16, 16, 0}, DET_BATCH}}},
    // C = 640: 256 / 2048 / 4096 rows and 16 frames; 32768 rows: the long-K (3200) folded FeedForward GEMM fills the chip with 256-row tiles (gemm8p.hip)
    {"leaf_transformer640", {{{2, 2, 8, 8, 77}, PLAIN}, {{2, 1, 32, 32, 77}, PLAIN}, {{2, 2, 32, 32, 77}, PLAIN}, {{1, 16, 8, 8, 77}, PLAIN}, {{1, 16, 16, 16, 77}, PLAIN},
                             {{2, 16, 32, 32, 77}, PLAIN}}},
    {"leaf_temporal640", {{{1, 16, 8, 8, 0}, PLAIN}, {{1, 8, 8, 8, 0}, PLAIN}, {{1, 16, 4, 4, 0}, PLAIN}, {{1, 16, 8, 16, 0}, PLAIN}, {{1, 16, 16, 16, 0}, PLAIN}}},
    // C = 1280: 2048 rows (and the 256 rows of the small-M kernel)
    {"leaf_transformer1280", {{{2, 1, 32, 32, 77}, PLAIN}, {{1, 16, 8, 16, 77}, PLAIN}, {{2, 2, 8, 8, 77}, PLAIN}}},
    {"leaf_temporal1280", {{{1, 16, 8, 16, 0}, PLAIN}, {{1, 16, 4, 4, 0}, PLAIN}}},
    {"tiny_sgm", {{{2, 1, 16, 16, 7}, PLAIN}}},
    {"tiny_vae_dec", {{{2, 1, 8, 8, 0}, PLAIN}}},
    {"tiny_vae_enc", {{{2, 1, 64, 64, 0}, PLAIN}}},
    {"tiny_clip", {{{2, 1, 1, 77, 0}, PLAIN}}},
};

static std::vector<std::pair<std::string, Net>> read_schema(const char* path) {      // in file order
  FILE* f = fopen(path, "r");
  CHECK(f, "schema file");
  std::vector<std::pair<std::string, Net>> nets;
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
  return nets;
}

// --ops: one call per line and switch setting.  Kernel launches are no-ops under the stub, so one dummy block stands in for every tensor
static int run_ops(const char* path) {
  FILE* f = fopen(path, "r");
  CHECK(f, "shapes file");
  std::vector<std::string> lines;
  char line[512];
  while (fgets(line, sizeof(line), f))
    if (line[0] != '#' && line[0] != '\n') lines.emplace_back(line, strcspn(line, "\n"));
  fclose(f);
  alignas(256) static char blk[4096];
  const float* fp = reinterpret_cast<const float*>(blk);
  for (int g8p = 0; g8p <= 2; ++g8p)
    for (const char* sm : {"", "0", "2"}) {
      nr_g8p_set_mode(g8p);
      if (*sm) setenv("NR_SMALLM", sm, 1); else unsetenv("NR_SMALLM");
      nr_stub_note(("== gemm8p mode " + std::to_string(g8p) + " NR_SMALLM=" + (*sm ? sm : "unset")).c_str());
      for (const std::string& l : lines) {
        nr_stub_note(l.c_str());
        char hook[32];
        int v[12] = {0};
        float scale = 1.f;
        nr_status st = NR_OK;
        if (sscanf(l.c_str(), "%31s", hook) != 1) continue;
        const std::string h = hook;
        if (h == "conv3x3") {
          CHECK(sscanf(l.c_str(), "%*s %d %d %d %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10) == 11, l.c_str());
          st = nr_op_conv3x3(nullptr, blk, v[3], v[4] ? blk : nullptr, v[4], v[0], v[1], v[2], v[6], v[7], blk, v[8] ? fp : nullptr, v[9] ? fp : nullptr, v[9], v[10] ? blk : nullptr, blk, v[5]);
        } else if (h == "conv3x3_tap_inner") {
          CHECK(sscanf(l.c_str(), "%*s %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7) == 8, l.c_str());
          st = nr_op_conv3x3_tap_inner(nullptr, blk, v[3], v[0], v[1], v[2], blk, v[5] ? fp : nullptr, v[6] ? fp : nullptr, v[6], v[7] ? blk : nullptr, blk, v[4]);
        } else {
          CHECK(sscanf(l.c_str(), "%*s %d %d %d %d %d %d %d %d %f %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, &scale, v + 8, v + 9, v + 10) == 12, l.c_str());
          const int M = v[0], N = v[1], K = v[2], bias = v[3], ln = v[4], res = v[5], geglu = v[6], act = v[7], rvd = v[8], rvm = v[9], c1 = v[10];
          const int No = geglu ? N / 2 : N;
          if (h == "gemm") st = nr_op_gemm(nullptr, blk, K, blk, bias ? fp : nullptr, res ? blk : nullptr, No, blk, No, M, N, K, geglu);
          else if (h == "gemm2") st = nr_op_gemm2(nullptr, blk, K - c1, K - c1, blk, c1, c1, blk, bias ? fp : nullptr, res ? blk : nullptr, N, blk, N, M, N);
          else if (h == "ln_gemm") st = nr_op_ln_gemm(nullptr, blk, K, blk, fp, fp, 1e-5f, res ? blk : nullptr, res ? No : 0, blk, No, M, N, K, geglu, act);
          else if (h == "gemm_ex") st = nr_op_gemm_ex(nullptr, blk, K, blk, bias ? fp : nullptr, ln ? fp : nullptr, 1e-5f, rvd ? fp : nullptr, rvd ? rvd : 1, rvm, rvd ? N : 0, res ? blk : nullptr, N, blk, N, M, N, K, 0, act, scale);
          else CHECK(false, l.c_str());
        }
        if (st != NR_OK) nr_stub_note(("status " + std::to_string((int)st)).c_str());
      }
    }
  return 0;
}

// --force-sweep: see the usage text.  M <= 512 rows, so of the five GEMM classes only smallm could claim a call, and it steps aside under NR_IGEMM_FORCE.
// The note is nr_gemm_route on the NrGemmParams the hook builds from the same arguments (engine_ops.hip); a hook that fails adds a "status" note
static int run_force_sweep() {
  alignas(256) static char blk[4096];
  const bf16* b = reinterpret_cast<const bf16*>(blk);
  bf16* o = reinterpret_cast<bf16*>(blk);
  const float* fp = reinterpret_cast<const float*>(blk);
  const int M = 320, N = 320, K = 256, H = 16, Cin = 64;      // Linears: 320 rows; convs: one 16 x 16 image (the phase form: 8 x 8 -> 16 x 16)
  struct Kind { const char* name; NrGemmParams p; std::function<nr_status()> hook; };
  std::vector<Kind> kinds;
  const auto linear = [&](const char* name, int geglu, bool ln) {
    const int Nw = geglu ? 2 * N : N;
    NrGemmParams p = nr_gemm_params(b, K, K, nullptr, 0, 0, M, 1, 1, 1, 1, 0, b, Nw, fp, b, N, o, N);
    p.geglu = geglu;
    if (ln) { p.ln_c = fp; p.ln_eps = 1e-5f; }
    kinds.push_back({name, p, [=]() { return ln ? nr_op_ln_gemm(nullptr, blk, K, blk, fp, fp, 1e-5f, blk, N, blk, N, M, Nw, K, geglu, 0)
                                                 : nr_op_gemm(nullptr, blk, K, blk, fp, blk, N, blk, N, M, Nw, K, geglu); }});
  };
  linear("linear", 0, false);
  linear("geglu", 1, false);
  linear("ln_linear", 0, true);
  linear("ln_geglu", 1, true);
  for (int c1 : {0, 2 * Cin}) {      // two sources of 128 channels: K = 2304, long enough for the heuristic's split-K (and its reduce launch)
    const int c0 = c1 ? c1 : Cin;
    NrGemmParams p = nr_gemm_params(b, c0, c0, c1 ? b : nullptr, c1, c1, 1, H, H, 3, 1, 0, b, N, fp, nullptr, N, o, N);
    kinds.push_back({c1 ? "conv3x3_2src" : "conv3x3", p, [=]() { return nr_op_conv3x3(nullptr, blk, c0, c1 ? blk : nullptr, c1, 1, H, H, 1, 0, blk, fp, nullptr, 0, nullptr, blk, N); }});
  }
  kinds.push_back({"conv3x3_ups_phase", nr_gemm_params(b, Cin, Cin, nullptr, 0, 0, 1, H / 2, H / 2, 3, 1, 2, b, N, fp, nullptr, 0, o, N),
                   [=]() { return nr_op_conv3x3_ups_phase(nullptr, blk, Cin, 1, H / 2, H / 2, blk, fp, blk, N); }});
  for (int bm : {64, 128, 256})
    for (int bn : {32, 64, 128, 160})
      for (int st = 2; st <= 8; ++st)
        for (int wv : {-1, 4, 8, 41}) {
          const std::string force = std::to_string(bm) + "," + std::to_string(bn) + ",-1," + std::to_string(st) + ",-1," + std::to_string(wv);
          setenv("NR_IGEMM_FORCE", force.c_str(), 1);
          for (const Kind& k : kinds) {
            NrGemmRoute r;
            const int rc = nr_gemm_route(&k.p, &r);
            const TiledPlan& t = r.tiled;
            char note[256];
            snprintf(note, sizeof(note), "route %s force=%s status=%d class=%s bm=%d bn=%d splitk=%d stages=%d waves=%d adma=%d lin=%d", k.name, force.c_str(), rc,
                     nr_gemm_class_name[r.cls], t.bm, t.bn, t.splitk, t.stages, t.waves, t.adma, t.lin);
            nr_stub_note(note);
            const nr_status st_hook = k.hook();
            if (st_hook != NR_OK) nr_stub_note(("status " + std::to_string((int)st_hook)).c_str());
          }
        }
  unsetenv("NR_IGEMM_FORCE");
  return 0;
}

// --decide-once: see the usage text.  Prints the status of each replay
static int run_decide_once(const char* schema) {
  const auto nets = read_schema(schema);
  const Net* n = nullptr;
  for (auto& nn : nets) if (nn.first == "leaf_transformer1280") n = &nn.second;
  CHECK(n, "schema has no leaf_transformer1280");
  std::vector<float> io((size_t)8 << 20);
  nr_net* h = nullptr;
  OK(nr_net_create(&n->cfg, &h));
  load_all(h, *n, 3);
  OK(nr_net_set_graph(h, 0));
  nr_g8p_set_mode(2);
  OK(nr_net_plan(h, 1, 16, 8, 8, 77));
  nr_stub_note("replay first");          // also runs the context ops (text k|v projections), which later replays skip
  printf("replay first: status %d\n", (int)nr_leaf_forward(h, nullptr, io.data(), io.data() + (2 << 20), 77, io.data() + (4 << 20)));
  nr_stub_note("replay planned");
  printf("replay planned: status %d\n", (int)nr_leaf_forward(h, nullptr, io.data(), io.data() + (2 << 20), 77, io.data() + (4 << 20)));
  nr_g8p_set_mode(1);
  setenv("NR_IGEMM_FORCE", "64,64,4,2,0", 1);
  nr_stub_note("replay switched");
  printf("replay switched: status %d (%s)\n", (int)nr_leaf_forward(h, nullptr, io.data(), io.data() + (2 << 20), 77, io.data() + (4 << 20)), nr_last_error());
  // the control: the same shape planned afresh under mode 1 takes the tiled kernel with split-K
  unsetenv("NR_IGEMM_FORCE");
  OK(nr_net_plan(h, 1, 16, 8, 8, 77));
  nr_stub_note("replay control");
  printf("replay control: status %d\n", (int)nr_leaf_forward(h, nullptr, io.data(), io.data() + (2 << 20), 77, io.data() + (4 << 20)));
  nr_net_destroy(h);
  return 0;
}

// --ff-waves: see the usage text.  Prints the status of each replay
static int run_ff_waves(const char* schema) {
  const auto nets = read_schema(schema);
  std::vector<float> io((size_t)8 << 20);
  const struct { const char* net; Shape s; } leaves[] = {{"leaf_temporal", {1, 16, 16, 16, 0}}, {"leaf_transformer", {1, 4, 32, 32, 77}}};
  for (const auto& lf : leaves) {
    const Net* n = nullptr;
    for (auto& nn : nets) if (nn.first == lf.net) n = &nn.second;
    CHECK(n, "schema lacks a C = 320 leaf");
    nr_net* h = nullptr;
    OK(nr_net_create(&n->cfg, &h));
    load_all(h, *n, 3);
    OK(nr_net_set_graph(h, 0));
    const auto replay = [&](const char* which) {
      nr_stub_note((std::string("replay ") + which + " " + lf.net).c_str());
      const nr_status st = nr_leaf_forward(h, nullptr, io.data(), lf.s.ctx ? io.data() + (2 << 20) : nullptr, lf.s.ctx, io.data() + (4 << 20));
      printf("replay %s %s: status %d\n", which, lf.net, (int)st);
    };
    nr_ff_set_waves(8);
    OK(nr_net_plan(h, lf.s.b, lf.s.f, lf.s.h, lf.s.w, lf.s.ctx));
    replay("first");          // also runs the context ops, which later replays skip
    replay("planned");
    nr_ff_set_waves(4);
    replay("switched");
    OK(nr_net_plan(h, lf.s.b, lf.s.f, lf.s.h, lf.s.w, lf.s.ctx));      // the control: planned afresh under 4 waves
    replay("control");
    nr_net_destroy(h);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: plan_dump <schema-file> [name,name,...] | --ops <shapes-file> | --decide-once <schema-file> | --ff-waves <schema-file> | --force-sweep\n"); return 1; }
  if (argc == 2 && std::string(argv[1]) == "--force-sweep") return run_force_sweep();
  if (argc == 3 && std::string(argv[1]) == "--ff-waves") return run_ff_waves(argv[2]);
  if (argc == 3 && std::string(argv[1]) == "--ops") return run_ops(argv[2]);
  if (argc == 3 && std::string(argv[1]) == "--decide-once") return run_decide_once(argv[2]);
  const std::string only = argc > 2 ? std::string(",") + argv[2] + "," : std::string();
  const std::vector<std::pair<std::string, Net>> nets = read_schema(argv[1]);
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
