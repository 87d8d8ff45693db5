// Denoiser-network engine behind the C ABI of include/neurons_amd.h.
//
// A handle owns (1) the state dict as loaded (host fp32, reference key names), (2) the converted
// device weights (bf16, layouts the kernels want: tap-major conv weights, fused q|k|v, GEGLU
// value/gate interleave, one concatenated time-embedding projection), (3) a launch plan: a flat
// list of kernel launches over one workspace arena with plan-time buffer reuse, (4) optionally that
// plan captured as a hipGraph.  forward() allocates nothing.
//
// This file: the graph-replay runtime of a handle, the C ABI, and the engine's two small kernels.  engine.h says where the rest lives.
#include "engine.h"

using namespace nre;

namespace {

thread_local std::string g_err;

__global__ void copy16_kernel(const uint4* __restrict__ a, uint4* __restrict__ b, long long n16) {   // debug snapshots only
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n16) b[i] = a[i];
}

struct TimestepVals { float v[NR_MAX_BATCH]; };
__global__ void set_timesteps_kernel(float* dst, TimestepVals tv, int n) {
  if (threadIdx.x < n) dst[threadIdx.x] = tv.v[threadIdx.x];
}

}  // namespace

void nre::set_err(const std::string& s) { g_err = s; }
void nre::launch_copy16(const void* src, void* dst, size_t nbytes, hipStream_t s) {
  const long long n16 = (long long)(nbytes / 16);
  hipLaunchKernelGGL(copy16_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, n16);
}

// ================================================================================================
// runtime
// ================================================================================================
nr_net::~nr_net() {
  if (arena_base) (void)hipFree(arena_base);
  drop_graphs();
  for (auto& e : ev_slot) if (e) (void)hipEventDestroy(e);
  if (ev_in) (void)hipEventDestroy(ev_in);
  if (ev_out) (void)hipEventDestroy(ev_out);
  if (ev_adds) (void)hipEventDestroy(ev_adds);
  if (own_stream) (void)hipStreamDestroy(own_stream);
}

void nr_net::drop_graphs() {
  for (auto& c : gcache) { for (auto& g : c) if (g.exec) (void)hipGraphExecDestroy(g.exec); c.clear(); }
}

void nr_net::ensure_streams() {
  if (!own_stream) {
    // (a lowest-priority stream for SparseCtrl, meant to fill only the CUs the U-Net leaves free, measured neutral: 16.56 vs 16.53 frames/s)
    // NR_STREAM_PRIO=1 (A/B): SparseCtrl on the lowest-priority queue, the U-Net on the highest, so that under the grouped schedule the
    // pending group only takes the CUs the U-Net's small launches leave free
    static const bool prio = env_is_1("NR_STREAM_PRIO");
    if (prio) {
      int lo = 0, hi = 0;
      HIP_OK(hipDeviceGetStreamPriorityRange(&lo, &hi));     // lo = numerically greatest = lowest priority
      HIP_OK(hipStreamCreateWithPriority(&own_stream, hipStreamNonBlocking, cfg.kind == NR_KIND_SPARSECTRL ? lo : hi));
    } else {
      HIP_OK(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
    }
    HIP_OK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&ev_adds, hipEventDisableTiming));
    for (auto& e : ev_slot) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
}
void nr_net::run_context(hipStream_t s) {
  if (!ctx_dirty) return;
  for (auto& op : ctx_ops) op(s);
  ctx_dirty = false;
}
void nr_net::set_timesteps(hipStream_t s, const float* timesteps) {
  TimestepVals tv;
  for (int i = 0; i < NR_MAX_BATCH; ++i) tv.v[i] = i < B2 ? timesteps[i] : 0.f;
  hipLaunchKernelGGL(set_timesteps_kernel, dim3(1), dim3(64), 0, s, t_dev, tv, B2);
}
// launch ops [begin, end) of segment `seg` on `s` as a (re)captured hipGraph
void nr_net::launch_segment(hipStream_t s, int seg) {
  const size_t begin = seg == 0 ? 0 : (seg == 1 ? split_op : split_op2);
  const size_t end = seg == 0 ? split_op : (seg == 1 ? split_op2 : ops.size());
  if (begin >= end) return;
  auto& cache = gcache[seg];
  // key = the IO fields this segment's kernels read: only segment 1 (the ControlNet-residual adds) sees the residual pointers, so the
  // encoder / decoder graphs of the U-Net are shared by every (slot, phase) of the grouped SparseCtrl schedule instead of being
  // captured once per residual-buffer set
  IO key = io;
  if (seg != 1 && cfg.kind == NR_KIND_UNET3D) {
    std::memset((void*)key.down_res, 0, sizeof(key.down_res));
    key.mid_res = nullptr;
    key.has_res = 0;
  }
  GraphSlot* hit = nullptr;
  for (auto& g : cache) if (g.exec && g.io == key) { hit = &g; break; }
  if (!hit) {
    if ((int)cache.size() >= NR_GRAPH_SLOTS) {              // evict the least recently used graph
      size_t lru = 0;
      for (size_t i = 1; i < cache.size(); ++i) if (cache[i].used < cache[lru].used) lru = i;
      HIP_OK(hipDeviceSynchronize());                        // it may still be executing, on this or on another stream
      (void)hipGraphExecDestroy(cache[lru].exec);
      cache.erase(cache.begin() + lru);
    }
    hipGraph_t g = nullptr;
    HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    try {
      for (size_t i = begin; i < end; ++i) ops[i](s);
    } catch (...) {
      (void)hipStreamEndCapture(s, &g);
      if (g) (void)hipGraphDestroy(g);
      throw;
    }
    HIP_OK(hipStreamEndCapture(s, &g));
    hipGraphExec_t ex = nullptr;
    hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) throw NrError(NR_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    GraphSlot gs; gs.io = key; gs.exec = ex;
    cache.push_back(gs);
    hit = &cache.back();
  }
  hit->used = ++gclock;
  HIP_OK(hipGraphLaunch(hit->exec, s));
}

void nr_net::run_eager(hipStream_t s, const float* timesteps) {
  begin(s, timesteps);
  for (auto& op : ops) op(s);
}
// graph mode: the engine's own stream, fenced behind everything the caller enqueued so far (readers of the buffers, staged inputs)
hipStream_t nr_net::begin_fenced(hipStream_t caller, const float* timesteps) {
  HIP_OK(hipEventRecord(ev_in, caller));
  HIP_OK(hipStreamWaitEvent(own_stream, ev_in, 0));
  begin(own_stream, timesteps);
  return own_stream;
}

void nr_net::run(hipStream_t caller, const float* timesteps) {
  if (!use_graph) {
    static const bool trace = getenv("NR_TRACE_OPS") != nullptr;      // fault localisation: one line and one stream sync per launch (eager handles only)
    if (trace) {
      begin(caller, timesteps);
      for (size_t i = 0; i < ops.size(); ++i) {
        fprintf(stderr, "[nr op %zu] %s\n", i, op_meta[i].desc.c_str());
        ops[i](caller);
        HIP_OK(hipStreamSynchronize(caller));
      }
      return;
    }
    run_eager(caller, timesteps);
    return;
  }
  ensure_streams();
  hipStream_t s = begin_fenced(caller, timesteps);
  launch_segment(s, 0);
  launch_segment(s, 1);
  launch_segment(s, 2);
  HIP_OK(hipEventRecord(ev_out, s));
  HIP_OK(hipStreamWaitEvent(caller, ev_out, 0));
}

// ================================================================================================
// C ABI
// ================================================================================================
static void profile_last(nr_net* h, hipStream_t s, nr_profile* out, const char* csv_path = nullptr) {
  std::memset(out, 0, sizeof(*out));
  const size_t n = h->ops.size();
  std::vector<hipEvent_t> ev(n + 1);
  for (auto& e : ev) HIP_OK(hipEventCreate(&e));
  HIP_OK(hipStreamSynchronize(s));
  HIP_OK(hipEventRecord(ev[0], s));
  for (size_t i = 0; i < n; ++i) {
    h->ops[i](s);
    HIP_OK(hipEventRecord(ev[i + 1], s));
  }
  HIP_OK(hipStreamSynchronize(s));
  FILE* f = csv_path ? fopen(csv_path, "w") : nullptr;
  if (f) fprintf(f, "idx,kind,ms,gflop,mbytes,desc\n");
  for (size_t i = 0; i < n; ++i) {
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
    const auto& m = h->op_meta[i];
    out->ms[m.kind] += ms; out->flops[m.kind] += m.flops; out->bytes[m.kind] += m.bytes; out->launches[m.kind] += m.launches;
    if (f) fprintf(f, "%zu,%d,%.4f,%.3f,%.3f,%s\n", i, m.kind, ms, m.flops / 1e9, m.bytes / 1e6, m.desc.c_str());
  }
  if (f) fclose(f);
  for (auto& e : ev) (void)hipEventDestroy(e);
}

extern "C" const char* nr_last_error(void) { return g_err.c_str(); }

// what nr_net_create accepts
static void check_config(const nr_net_config* cfg) {
  if (cfg->kind < NR_KIND_UNET3D || cfg->kind > NR_KIND_LEAF_TEMPORAL) throw NrError(NR_ERR_ARG, "bad kind");
  const bool leaf_kind = cfg->kind == NR_KIND_LEAF_TRANSFORMER3D || cfg->kind == NR_KIND_LEAF_TEMPORAL;
  if (cfg->num_levels < (leaf_kind ? 1 : 2) || cfg->num_levels > NR_MAX_LEVELS) throw NrError(NR_ERR_ARG, "num_levels must be 2..4");
  if (cfg->kind == NR_KIND_CLIP_TEXT) {
    const int C = cfg->block_out_channels[0];
    if (C % 64 != 0 || cfg->num_heads <= 0 || C % cfg->num_heads != 0 || (C / cfg->num_heads) % 8 != 0 || C / cfg->num_heads > 160 ||
        cfg->cross_attention_dim % 64 != 0 || cfg->in_channels <= 0 || cfg->layers_per_block <= 0 || cfg->motion_pe_max_len <= 0)
      throw NrError(NR_ERR_UNSUPPORTED, "CLIP text encoder: hidden/intermediate sizes must be multiples of 64, head dim a multiple of 8 and <= 160");
    return;
  }
  const bool vae = cfg->kind == NR_KIND_VAE_DECODER || cfg->kind == NR_KIND_VAE_ENCODER;
  if (cfg->kind == NR_KIND_VAE_DECODER && (cfg->in_channels != 4 || cfg->out_channels != 3))
    throw NrError(NR_ERR_UNSUPPORTED, "VAE decoder: z_channels must be 4 and out_ch 3");
  if (cfg->kind == NR_KIND_VAE_ENCODER && (cfg->in_channels != 3 || cfg->out_channels != 8))
    throw NrError(NR_ERR_UNSUPPORTED, "VAE encoder: in_channels must be 3 and the moments 2 * z_channels = 8");
  for (int i = 0; i < cfg->num_levels; ++i) {
    const int C = cfg->block_out_channels[i];
    if (C % 64 != 0) throw NrError(NR_ERR_UNSUPPORTED, "block_out_channels must be multiples of 64");
    if (C % cfg->norm_num_groups != 0) throw NrError(NR_ERR_ARG, "channels not divisible by norm_num_groups");
    const int hd = cfg->num_head_channels > 0 ? cfg->num_head_channels : (cfg->num_heads > 0 ? C / cfg->num_heads : 0);
    if (!vae && (hd <= 0 || C % hd != 0 || hd % 8 != 0 || hd > 160))
      throw NrError(NR_ERR_UNSUPPORTED, "head dim must divide the channels, be a multiple of 8 and <= 160");
  }
  if (!vae && cfg->cross_attention_dim % 64 != 0) throw NrError(NR_ERR_UNSUPPORTED, "cross_attention_dim must be a multiple of 64");
  if (cfg->norm_num_groups > 64) throw NrError(NR_ERR_UNSUPPORTED, "norm_num_groups > 64");
  if (cfg->kind == NR_KIND_SPARSECTRL && cfg->cond_embedding_levels != 0) {
    const int L = cfg->cond_embedding_levels;
    const int* ch = cfg->cond_embedding_channels;
    bool ok = L >= 1 && L <= NR_MAX_LEVELS && nr_condembed_in_supported(cfg->conditioning_channels + 1, ch[0]);
    for (int i = 0; ok && i + 1 < L; ++i) ok = nr_condembed_conv_supported(ch[i], 1, ch[i]) && nr_condembed_conv_supported(ch[i], 2, ch[i + 1]);
    if (ok && ch[L - 1] % 64 != 0) ok = nr_condembed_conv_supported(ch[L - 1], 1, cfg->block_out_channels[0]);
    if (!ok)
      throw NrError(NR_ERR_UNSUPPORTED, "SparseCtrl condition embedding: 1..4 levels, conditioning_channels + 1 <= 8, first level 16 or 32 "
                                        "channels, the others 16 / 32 / 64 / 96 / 128 / 256");
  }
}

extern "C" nr_status nr_net_create(const nr_net_config* cfg, nr_net** out) {
  NR_TRY
  if (!cfg || !out) throw NrError(NR_ERR_ARG, "null argument");
  check_config(cfg);
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) throw NrError(NR_ERR_HIP, "no HIP device available: libneurons_amd requires an MI355X (gfx950) GPU");
  nr_net* h = new nr_net();
  h->cfg = *cfg;
  h->device = dev;
  h->det_batch = env_is_1("NR_DETERMINISTIC_BATCH");
  h->w8 = env_is_1("NR_W8");
  *out = h;
  NR_CATCH
}

extern "C" void nr_net_destroy(nr_net* h) { delete h; }

extern "C" nr_status nr_net_load_tensor(nr_net* h, const char* key, const float* host_data, const int64_t* shape, int32_t ndim) {
  NR_TRY
  if (!h || !key || !host_data || ndim < 0 || ndim > 8) throw NrError(NR_ERR_ARG, "bad argument");
  if (h->wts.load_tensor(key, host_data, shape, ndim)) h->planned = false;      // converted copies derived from this key were dropped
  NR_CATCH
}

// every entry point that allocates or launches runs on the CURRENT HIP device: it must be the one the handle was created on
static void check_device(const nr_net* h) {
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != h->device)
    throw NrError(NR_ERR_STATE, "handle was created on HIP device " + std::to_string(h->device) + " but device " + std::to_string(cur) +
                                    " is current (hipSetDevice / torch.cuda.device before calling)");
}

// common preamble of the forward entry points: a handle of an accepted kind, planned (not_planned = null: not required), on the current device
static void check_forward(const nr_net* h, std::initializer_list<int> kinds, const char* not_kind,
                          const char* not_planned = "nr_net_plan() has not been called (or weights changed since)") {
  if (!h || std::find(kinds.begin(), kinds.end(), (int)h->cfg.kind) == kinds.end()) throw NrError(NR_ERR_ARG, not_kind);
  if (not_planned && !h->planned) throw NrError(NR_ERR_STATE, not_planned);
  check_device(h);
}

extern "C" nr_status nr_net_plan(nr_net* h, int32_t batch, int32_t frames, int32_t lat_h, int32_t lat_w, int32_t ctx_len) {
  NR_TRY
  if (!h) throw NrError(NR_ERR_ARG, "null handle");
  check_device(h);
  h->plan(batch, frames, lat_h, lat_w, ctx_len);
  NR_CATCH
}

// ---- converted-weight exchange between handles (WeightStore::manifest / export_to / import_from) ----
extern "C" int64_t nr_net_export_manifest(nr_net* h, char* buf, int64_t capacity, int64_t* arena_bytes) {
  if (!h || !h->planned) { set_err("nr_net_export_manifest: plan first (the converted buffers are created by nr_net_plan)"); return -1; }
  size_t total = 0;
  const std::string m = h->wts.manifest(h->cfg.kind, &total);
  if (arena_bytes) *arena_bytes = (int64_t)total;
  if (buf && capacity >= (int64_t)m.size()) std::memcpy(buf, m.data(), m.size());
  return (int64_t)m.size();
}

extern "C" nr_status nr_net_export_weights(nr_net* h, nr_stream stream, void* dst_dev, int64_t capacity) {
  NR_TRY
  if (!h || !dst_dev) throw NrError(NR_ERR_ARG, "null argument");
  if (!h->planned) throw NrError(NR_ERR_STATE, "plan first");
  check_device(h);
  size_t total = 0;
  (void)h->wts.manifest(h->cfg.kind, &total);
  if ((size_t)capacity < total) throw NrError(NR_ERR_ARG, "export buffer too small");
  h->wts.export_to(dst_dev, (hipStream_t)stream);
  NR_CATCH
}

extern "C" nr_status nr_net_import_weights(nr_net* h, nr_stream stream, const char* manifest, int64_t manifest_bytes, const void* src_dev,
                                           int64_t arena_bytes) {
  NR_TRY
  if (!h || !manifest || !src_dev) throw NrError(NR_ERR_ARG, "null argument");
  check_device(h);
  h->wts.import_from(h->cfg.kind, std::string(manifest, (size_t)manifest_bytes), src_dev, arena_bytes, (hipStream_t)stream);
  NR_CATCH
}

extern "C" nr_status nr_net_release_host_weights(nr_net* h) {
  NR_TRY
  if (!h) throw NrError(NR_ERR_ARG, "null handle");
  if (!h->planned) throw NrError(NR_ERR_STATE, "plan first: the converted device copies must exist");
  h->wts.release_host();
  NR_CATCH
}

extern "C" nr_status nr_net_invalidate_context(nr_net* h) {
  NR_TRY
  if (!h) throw NrError(NR_ERR_ARG, "null handle");
  h->ctx_dirty = true;
  h->prefetch_valid = false;
  NR_CATCH
}

extern "C" nr_status nr_net_set_graph(nr_net* h, int32_t enable) {
  NR_TRY
  if (!h) throw NrError(NR_ERR_ARG, "null handle");
  h->use_graph = enable != 0;
  NR_CATCH
}

extern "C" nr_status nr_sparsectrl_set_condition_frames(nr_net* h, const int32_t* frames, int32_t n) {
  NR_TRY
  if (!h || h->cfg.kind != NR_KIND_SPARSECTRL) throw NrError(NR_ERR_ARG, "handle is not a SparseCtrl");
  if (n > 64 || (n > 0 && !frames)) throw NrError(NR_ERR_ARG, "at most 64 condition frames");
  int v[64] = {0};
  int m = n < 0 ? -1 : 0;
  for (int i = 0; i < n; ++i) {
    if (frames[i] < 0) throw NrError(NR_ERR_ARG, "negative frame index");
    bool dup = false;
    for (int k = 0; k < m; ++k) dup = dup || v[k] == frames[i];
    if (!dup) v[m++] = frames[i];
  }
  bool same = m == h->n_cond_frames;
  for (int i = 0; same && i < m; ++i) same = v[i] == h->cond_frames[i];
  if (!same) {
    h->n_cond_frames = m;
    for (int i = 0; i < 64; ++i) h->cond_frames[i] = i < m ? v[i] : 0;
    h->planned = false;
  }
  NR_CATCH
}

extern "C" nr_status nr_net_set_deterministic_batch(nr_net* h, int32_t enable) {
  NR_TRY
  if (!h) throw NrError(NR_ERR_ARG, "null handle");
  if (h->det_batch != (enable != 0)) { h->det_batch = enable != 0; h->planned = false; }
  NR_CATCH
}

extern "C" nr_status nr_net_set_clip_samples(nr_net* h, int32_t samples) {
  NR_TRY
  if (!h) throw NrError(NR_ERR_ARG, "null handle");
  if (samples != 1 && samples != 2) throw NrError(NR_ERR_ARG, "clip samples must be 1 (no guidance) or 2 (CFG pair)");
  if (h->clip_samples != samples) { h->clip_samples = samples; if (h->det_batch) h->planned = false; }
  NR_CATCH
}

extern "C" nr_status nr_net_set_cfg_pair_identical(nr_net* h, int32_t enable) {
  NR_TRY
  if (!h) throw NrError(NR_ERR_ARG, "null handle");
  if (h->cfg_dup != (enable != 0)) { h->cfg_dup = enable != 0; h->planned = false; }
  NR_CATCH
}

extern "C" nr_status nr_net_set_attention_fp8(nr_net* h, int32_t enable) {
  NR_TRY
  if (!h) throw NrError(NR_ERR_ARG, "null handle");
  if (h->attn_fp8 != (enable != 0)) { h->attn_fp8 = enable != 0; h->planned = false; }
  NR_CATCH
}

extern "C" nr_status nr_net_set_weight_fp8(nr_net* h, int32_t enable) {
  NR_TRY
  if (!h) throw NrError(NR_ERR_ARG, "null handle");
  if (h->w8 != (enable != 0)) { h->w8 = enable != 0; h->planned = false; }
  NR_CATCH
}

extern "C" nr_status nr_net_set_debug(nr_net* h, int32_t keep) {
  NR_TRY
  if (!h) throw NrError(NR_ERR_ARG, "null handle");
  h->keep_all = keep != 0;
  h->planned = false;
  NR_CATCH
}

extern "C" int64_t nr_net_workspace_bytes(const nr_net* h) { return h ? (int64_t)h->arena_bytes : 0; }
extern "C" int64_t nr_net_weight_bytes(const nr_net* h) { return h ? (int64_t)h->wts.weight_bytes : 0; }
extern "C" int32_t nr_net_num_residuals(const nr_net* h) { return h ? h->n_res : 0; }
extern "C" nr_status nr_net_residual_shape(const nr_net* h, int32_t i, int32_t* C, int32_t* hh, int32_t* ww) {
  NR_TRY
  if (!h || !h->planned) throw NrError(NR_ERR_STATE, "not planned");
  if (i < 0 || i >= (int)h->res_shapes.size()) throw NrError(NR_ERR_ARG, "residual index out of range");
  *C = h->res_shapes[i].C; *hh = h->res_shapes[i].h; *ww = h->res_shapes[i].w;
  NR_CATCH
}

extern "C" nr_status nr_unet3d_forward(nr_net* h, nr_stream stream, const float* sample_dev, const float* timesteps,
                                       const float* ctx_dev, int32_t ctx_len, const void* const* down_res_dev,
                                       const void* mid_res_dev, float* out_dev) {
  NR_TRY
  check_forward(h, {NR_KIND_UNET3D}, "handle is not a UNet3D");
  if (!sample_dev || !timesteps || !ctx_dev || !out_dev) throw NrError(NR_ERR_ARG, "null tensor argument");
  if (ctx_len != h->ctx_len) throw NrError(NR_ERR_ARG, "ctx_len differs from the planned value");
  if ((down_res_dev == nullptr) != (mid_res_dev == nullptr)) throw NrError(NR_ERR_ARG, "down/mid residuals must be given together");
  IO io = new_io();
  io.sample = sample_dev; io.ctx = ctx_dev; io.out = out_dev;
  if (down_res_dev) {
    io.has_res = 1;
    for (int i = 0; i < h->n_res; ++i) {
      if (!down_res_dev[i]) throw NrError(NR_ERR_ARG, "null residual pointer");
      io.down_res[i] = down_res_dev[i];
    }
    io.mid_res = mid_res_dev;
  }
  h->io = io;
  h->run((hipStream_t)stream, timesteps);
  NR_CATCH
}

extern "C" nr_status nr_sparsectrl_forward(nr_net* h, nr_stream stream, const float* sample_dev, const float* timesteps,
                                           const float* ctx_dev, int32_t ctx_len, const float* cond_dev,
                                           const float* mask_dev, int32_t cond_batch, float scale,
                                           void* const* out_down_dev, void* out_mid_dev) {
  NR_TRY
  check_forward(h, {NR_KIND_SPARSECTRL}, "handle is not a SparseCtrl");
  if (!timesteps || !ctx_dev || !cond_dev || !mask_dev || !out_down_dev || !out_mid_dev) throw NrError(NR_ERR_ARG, "null tensor argument");
  if (!h->cfg.set_noisy_sample_input_to_zero && !sample_dev) throw NrError(NR_ERR_ARG, "sample required");
  if (ctx_len != h->ctx_len) throw NrError(NR_ERR_ARG, "ctx_len differs from the planned value");
  if (cond_batch <= 0 || h->B2 % cond_batch != 0) throw NrError(NR_ERR_ARG, "cond_batch must divide the planned batch");
  IO io = new_io();
  io.sample = sample_dev; io.ctx = ctx_dev; io.cond = cond_dev; io.mask = mask_dev; io.cond_batch = cond_batch; io.scale = scale;
  for (int i = 0; i < h->n_res; ++i) {
    if (!out_down_dev[i]) throw NrError(NR_ERR_ARG, "null output pointer");
    io.out_down[i] = out_down_dev[i];
  }
  io.out_mid = out_mid_dev;
  h->io = io;
  h->run((hipStream_t)stream, timesteps);
  NR_CATCH
}

extern "C" nr_status nr_denoise_step_forward(nr_net* unet, nr_net* ctrl, nr_stream stream, const float* sample_dev,
                                             const float* timesteps, const float* ctx_dev, int32_t ctx_len,
                                             const float* cond_dev, const float* mask_dev, int32_t cond_batch, float scale,
                                             void* const* res_down_dev, void* res_mid_dev, float* out_dev,
                                             const float* next_timesteps) {
  NR_TRY
  check_forward(unet, {NR_KIND_UNET3D}, "need a UNet3D and a SparseCtrl handle", "nr_net_plan() has not been called on both handles");
  check_forward(ctrl, {NR_KIND_SPARSECTRL}, "need a UNet3D and a SparseCtrl handle", "nr_net_plan() has not been called on both handles");
  if (!sample_dev || !timesteps || !ctx_dev || !cond_dev || !mask_dev || !res_down_dev || !res_mid_dev || !out_dev) throw NrError(NR_ERR_ARG, "null tensor argument");
  if (ctx_len != unet->ctx_len || ctx_len != ctrl->ctx_len) throw NrError(NR_ERR_ARG, "ctx_len differs from the planned value");
  if (unet->n_res != ctrl->n_res || unet->B2 != ctrl->B2 || unet->F != ctrl->F || unet->H != ctrl->H || unet->W != ctrl->W)
    throw NrError(NR_ERR_ARG, "the two handles are planned for different shapes");
  if (!ctrl->cfg.set_noisy_sample_input_to_zero) throw NrError(NR_ERR_UNSUPPORTED, "overlapped step requires set_noisy_sample_input_to_zero");
  if (cond_batch <= 0 || ctrl->B2 % cond_batch != 0) throw NrError(NR_ERR_ARG, "cond_batch must divide the planned batch");
  hipStream_t caller = (hipStream_t)stream;
  IO ic = new_io();
  ic.ctx = ctx_dev; ic.cond = cond_dev; ic.mask = mask_dev; ic.cond_batch = cond_batch; ic.scale = scale;
  IO iu = new_io();
  iu.sample = sample_dev; iu.ctx = ctx_dev; iu.out = out_dev; iu.has_res = 1;
  for (int i = 0; i < ctrl->n_res; ++i) {
    if (!res_down_dev[i]) throw NrError(NR_ERR_ARG, "null residual pointer");
    ic.out_down[i] = res_down_dev[i];
    iu.down_res[i] = res_down_dev[i];
  }
  ic.out_mid = res_mid_dev; iu.mid_res = res_mid_dev;
  ctrl->io = ic; unet->io = iu;
  if (!unet->use_graph || !ctrl->use_graph) {   // eager: plain sequential launches on the caller's stream
    ctrl->run_eager(caller, timesteps);
    unet->run_eager(caller, timesteps);
  } else {
    unet->ensure_streams(); ctrl->ensure_streams();
    HIP_OK(hipEventRecord(unet->ev_in, caller));
    HIP_OK(hipStreamWaitEvent(unet->own_stream, unet->ev_in, 0));
    // SparseCtrl on its stream — unless this step's evaluation was already issued by the previous call
    // (next_timesteps): with the noisy sample zeroed its inputs are (timestep, context, condition) only
    bool hit = ctrl->prefetch_valid && !ctrl->ctx_dirty && ctrl->prefetch_io == ic;
    for (int i = 0; hit && i < ctrl->B2; ++i) hit = ctrl->prefetch_t[i] == timesteps[i];
    ctrl->prefetch_valid = false;
    static const int dbg_mode = getenv("NR_OVERLAP_DBG") ? atoi(getenv("NR_OVERLAP_DBG")) : 0;   // 1: eager launches on the two streams; 2: graphs, serialised
    if (!hit) {
      HIP_OK(hipStreamWaitEvent(ctrl->own_stream, unet->ev_in, 0));
      ctrl->begin(ctrl->own_stream, timesteps);
      if (dbg_mode == 1) { for (auto& op : ctrl->ops) op(ctrl->own_stream); }
      else for (int seg = 0; seg < 3; ++seg) ctrl->launch_segment(ctrl->own_stream, seg);
      HIP_OK(hipEventRecord(ctrl->ev_out, ctrl->own_stream));
    }
    if (dbg_mode == 2) HIP_OK(hipStreamWaitEvent(unet->own_stream, ctrl->ev_out, 0));
    // ... concurrently with the U-Net's encoder + mid block; the residual adds wait for SparseCtrl
    unet->begin(unet->own_stream, timesteps);
    if (dbg_mode == 1) { for (size_t i = 0; i < unet->split_op; ++i) unet->ops[i](unet->own_stream); }
    else unet->launch_segment(unet->own_stream, 0);
    HIP_OK(hipStreamWaitEvent(unet->own_stream, ctrl->ev_out, 0));
    if (dbg_mode == 1) { for (size_t i = unet->split_op; i < unet->split_op2; ++i) unet->ops[i](unet->own_stream); }
    else unet->launch_segment(unet->own_stream, 1);
    HIP_OK(hipEventRecord(unet->ev_adds, unet->own_stream));
    if (dbg_mode == 1) { for (size_t i = unet->split_op2; i < unet->ops.size(); ++i) unet->ops[i](unet->own_stream); }
    else unet->launch_segment(unet->own_stream, 2);
    HIP_OK(hipEventRecord(unet->ev_out, unet->own_stream));
    HIP_OK(hipStreamWaitEvent(caller, unet->ev_out, 0));
    if (next_timesteps) {
      // the adds were the last readers of SparseCtrl's residual buffers: the next step's SparseCtrl evaluation can
      // start now and overlaps this step's decoder and the next step's encoder
      HIP_OK(hipStreamWaitEvent(ctrl->own_stream, unet->ev_adds, 0));
      ctrl->set_timesteps(ctrl->own_stream, next_timesteps);
      for (int seg = 0; seg < 3; ++seg) ctrl->launch_segment(ctrl->own_stream, seg);
      HIP_OK(hipEventRecord(ctrl->ev_out, ctrl->own_stream));
      ctrl->prefetch_valid = true;
      ctrl->prefetch_io = ic;
      for (int i = 0; i < NR_MAX_BATCH; ++i) ctrl->prefetch_t[i] = i < ctrl->B2 ? next_timesteps[i] : 0.f;
    }
  }
  NR_CATCH
}

// ---- grouped SparseCtrl schedule -----------------------------------------------------------------------------------------------
// With `set_noisy_sample_input_to_zero` (the NEURONS configuration, sparse_controlnet.py:469-470) SparseCtrl's inputs are the timestep, the
// text context and the condition: nothing of the denoising state.  Its evaluations for G consecutive DDIM steps can therefore run as ONE
// forward on a batch of G x (CFG batch), ahead of the U-Net that consumes them: the same 50 evaluations, at the GEMM efficiency of a G
// times larger M (5.64 -> 4.68 / 4.15 ms per step for G = 2 / 4, tools/ctrl_batch.py).  The caller (pipeline.py) owns the schedule:
//   nr_sparsectrl_forward_async  evaluates one group on the handle's own stream, NOT joined to the caller's stream, and records its
//                                completion in event slot 0/1;
//   nr_unet3d_forward_after      is nr_unet3d_forward whose residual adds wait for such a slot (its encoder overlaps the pending group).
extern "C" nr_status nr_sparsectrl_forward_async(nr_net* h, nr_stream stream, const float* timesteps, const float* ctx_dev, int32_t ctx_len,
                                                 const float* cond_dev, const float* mask_dev, int32_t cond_batch, float scale,
                                                 void* const* out_down_dev, void* out_mid_dev, int32_t slot) {
  NR_TRY
  check_forward(h, {NR_KIND_SPARSECTRL}, "handle is not a SparseCtrl");
  if (!h->cfg.set_noisy_sample_input_to_zero) throw NrError(NR_ERR_UNSUPPORTED, "the asynchronous evaluation requires set_noisy_sample_input_to_zero");
  if (!timesteps || !ctx_dev || !cond_dev || !mask_dev || !out_down_dev || !out_mid_dev) throw NrError(NR_ERR_ARG, "null tensor argument");
  if (ctx_len != h->ctx_len) throw NrError(NR_ERR_ARG, "ctx_len differs from the planned value");
  if (cond_batch <= 0 || h->B2 % cond_batch != 0) throw NrError(NR_ERR_ARG, "cond_batch must divide the planned batch");
  if (slot < 0 || slot > 1) throw NrError(NR_ERR_ARG, "slot must be 0 or 1");
  IO io = new_io();
  io.ctx = ctx_dev; io.cond = cond_dev; io.mask = mask_dev; io.cond_batch = cond_batch; io.scale = scale;
  for (int i = 0; i < h->n_res; ++i) {
    if (!out_down_dev[i]) throw NrError(NR_ERR_ARG, "null residual pointer");
    io.out_down[i] = out_down_dev[i];
  }
  io.out_mid = out_mid_dev;
  h->io = io;
  h->prefetch_valid = false;
  hipStream_t caller = (hipStream_t)stream;
  h->ensure_streams();
  if (!h->use_graph) {                       // eager handles: evaluate in stream order on the caller's stream
    h->run_eager(caller, timesteps);
    HIP_OK(hipEventRecord(h->ev_slot[slot], caller));
  } else {
    hipStream_t s = h->begin_fenced(caller, timesteps);
    for (int seg = 0; seg < 3; ++seg) h->launch_segment(s, seg);
    HIP_OK(hipEventRecord(h->ev_slot[slot], s));
  }
  NR_CATCH
}

extern "C" nr_status nr_unet3d_forward_after(nr_net* unet, nr_net* ctrl, int32_t slot, nr_stream stream, const float* sample_dev,
                                             const float* timesteps, const float* ctx_dev, int32_t ctx_len,
                                             const void* const* down_res_dev, const void* mid_res_dev, float* out_dev) {
  NR_TRY
  check_forward(unet, {NR_KIND_UNET3D}, "first handle is not a UNet3D");
  check_forward(ctrl, {NR_KIND_SPARSECTRL}, "second handle is not a SparseCtrl", nullptr);
  if (!sample_dev || !timesteps || !ctx_dev || !out_dev || !down_res_dev || !mid_res_dev) throw NrError(NR_ERR_ARG, "null tensor argument");
  if (ctx_len != unet->ctx_len) throw NrError(NR_ERR_ARG, "ctx_len differs from the planned value");
  if (slot < 0 || slot > 1) throw NrError(NR_ERR_ARG, "slot must be 0 or 1");
  if (unet->n_res != ctrl->n_res) throw NrError(NR_ERR_ARG, "the two handles have different residual counts");
  IO io = new_io();
  io.sample = sample_dev; io.ctx = ctx_dev; io.out = out_dev; io.has_res = 1;
  for (int i = 0; i < unet->n_res; ++i) {
    if (!down_res_dev[i]) throw NrError(NR_ERR_ARG, "null residual pointer");
    io.down_res[i] = down_res_dev[i];
  }
  io.mid_res = mid_res_dev;
  unet->io = io;
  hipStream_t caller = (hipStream_t)stream;
  unet->ensure_streams(); ctrl->ensure_streams();
  if (!unet->use_graph) {
    HIP_OK(hipStreamWaitEvent(caller, ctrl->ev_slot[slot], 0));
    unet->run_eager(caller, timesteps);
  } else {
    hipStream_t s = unet->begin_fenced(caller, timesteps);
    unet->launch_segment(s, 0);                                    // encoder + mid block: overlaps the pending SparseCtrl group
    HIP_OK(hipStreamWaitEvent(s, ctrl->ev_slot[slot], 0));
    unet->launch_segment(s, 1);                                    // the residual adds
    unet->launch_segment(s, 2);
    HIP_OK(hipEventRecord(unet->ev_out, s));
    HIP_OK(hipStreamWaitEvent(caller, unet->ev_out, 0));
  }
  NR_CATCH
}

extern "C" nr_status nr_sgm_unet_forward(nr_net* h, nr_stream stream, const float* x_dev, float in_scale, const float* timesteps,
                                         const float* ctx_dev, int32_t ctx_len, const float* y_dev, float* out_dev) {
  NR_TRY
  check_forward(h, {NR_KIND_SGM_UNET}, "handle is not an sgm UNetModel");
  if (!x_dev || !timesteps || !ctx_dev || !y_dev || !out_dev) throw NrError(NR_ERR_ARG, "null tensor argument");
  if (ctx_len != h->ctx_len) throw NrError(NR_ERR_ARG, "ctx_len differs from the planned value");
  IO io = new_io();
  io.sample = x_dev; io.ctx = ctx_dev; io.y = y_dev; io.out = out_dev; io.in_scale = in_scale;
  h->io = io;
  h->run((hipStream_t)stream, timesteps);
  NR_CATCH
}

extern "C" nr_status nr_leaf_forward(nr_net* h, nr_stream stream, const float* x_dev, const float* ctx_dev, int32_t ctx_len, float* out_dev) {
  NR_TRY
  check_forward(h, {NR_KIND_LEAF_TRANSFORMER3D, NR_KIND_LEAF_TEMPORAL}, "handle is not a leaf module");
  if (!x_dev || !out_dev) throw NrError(NR_ERR_ARG, "null tensor argument");
  if (h->cfg.kind == NR_KIND_LEAF_TRANSFORMER3D && (!ctx_dev || ctx_len != h->ctx_len)) throw NrError(NR_ERR_ARG, "context missing or ctx_len differs from the planned value");
  IO io = new_io();
  io.sample = x_dev; io.ctx = ctx_dev; io.out = out_dev;
  h->io = io;
  const float zeros[NR_MAX_BATCH] = {0};
  h->run((hipStream_t)stream, zeros);
  NR_CATCH
}

extern "C" int32_t nr_net_num_ops(const nr_net* h) { return h ? (int32_t)h->op_meta.size() : 0; }
extern "C" const char* nr_net_op_desc(const nr_net* h, int32_t i) {
  if (!h || i < 0 || i >= (int)h->op_meta.size()) return "";
  return h->op_meta[i].desc.c_str();
}

extern "C" nr_status nr_vae_decode(nr_net* h, nr_stream stream, const float* z_dev, float z_scale, float out_mul, float out_add,
                                   int32_t clamp01, float* out_dev) {
  NR_TRY
  check_forward(h, {NR_KIND_VAE_DECODER}, "handle is not a VAE decoder");
  if (!z_dev || !out_dev) throw NrError(NR_ERR_ARG, "null tensor argument");
  IO io = new_io();
  io.sample = z_dev; io.out = out_dev; io.in_scale = z_scale; io.out_mul = out_mul; io.out_add = out_add; io.clamp01 = clamp01 ? 1 : 0;
  h->io = io;
  const float zeros[NR_MAX_BATCH] = {0};
  h->run((hipStream_t)stream, zeros);
  NR_CATCH
}

extern "C" nr_status nr_clip_text_forward(nr_net* h, nr_stream stream, const int32_t* ids_dev, float* out_dev) {
  NR_TRY
  check_forward(h, {NR_KIND_CLIP_TEXT}, "handle is not a CLIP text encoder");
  if (!ids_dev || !out_dev) throw NrError(NR_ERR_ARG, "null tensor argument");
  IO io = new_io();
  io.ids = ids_dev; io.out = out_dev;
  h->io = io;
  const float zeros[NR_MAX_BATCH] = {0};
  h->run((hipStream_t)stream, zeros);
  NR_CATCH
}

extern "C" nr_status nr_vae_encode(nr_net* h, nr_stream stream, const float* x_dev, float in_mul, float in_add, float* moments_dev) {
  NR_TRY
  check_forward(h, {NR_KIND_VAE_ENCODER}, "handle is not a VAE encoder");
  if (!x_dev || !moments_dev) throw NrError(NR_ERR_ARG, "null tensor argument");
  IO io = new_io();
  io.sample = x_dev; io.out = moments_dev; io.in_scale = in_mul; io.in_shift = in_add;
  h->io = io;
  const float zeros[NR_MAX_BATCH] = {0};
  h->run((hipStream_t)stream, zeros);
  NR_CATCH
}

extern "C" nr_status nr_gaussian_sample(nr_stream stream, const float* moments_dev, const float* noise_dev, float* out_dev, int32_t n,
                                        int32_t z_channels, int32_t hw, float scale) {
  NR_TRY
  if (!moments_dev || !out_dev || n <= 0 || z_channels <= 0 || hw <= 0) throw NrError(NR_ERR_ARG, "bad argument");
  LAUNCH_OK(nr_launch_gaussian_sample(moments_dev, noise_dev, out_dev, n, z_channels, hw, scale, (hipStream_t)stream));
  NR_CATCH
}

extern "C" nr_status nr_net_profile_last(nr_net* h, nr_stream stream, nr_profile* out) {
  NR_TRY
  if (!h || !out) throw NrError(NR_ERR_ARG, "null argument");
  if (!h->planned || !(h->io.sample || h->io.ctx || h->io.ids)) throw NrError(NR_ERR_STATE, "run a forward first");
  profile_last(h, (hipStream_t)stream, out, getenv("NR_PROFILE_CSV"));
  NR_CATCH
}

extern "C" int32_t nr_net_num_taps(const nr_net* h) { return h ? (int32_t)h->taps.size() : 0; }
extern "C" const char* nr_net_tap_name(const nr_net* h, int32_t i) {
  if (!h || i < 0 || i >= (int)h->taps.size()) return "";
  return h->taps[i].name.c_str();
}
extern "C" nr_status nr_net_read_tap(nr_net* h, int32_t i, float* host_out, int64_t capacity, int32_t* rows, int32_t* C) {
  NR_TRY
  if (!h || i < 0 || i >= (int)h->taps.size()) throw NrError(NR_ERR_ARG, "tap index out of range");
  const Tap& t = h->taps[i];
  *rows = (int32_t)t.rows; *C = t.C;
  if (capacity < t.rows * t.C) throw NrError(NR_ERR_ARG, "tap buffer too small");
  HIP_OK(hipDeviceSynchronize());
  std::vector<uint16_t> tmp((size_t)t.rows * t.ld);
  HIP_OK(hipMemcpy(tmp.data(), t.ptr, tmp.size() * 2, hipMemcpyDeviceToHost));
  for (int64_t r = 0; r < t.rows; ++r)
    for (int c = 0; c < t.C; ++c) {
      const uint32_t u = (uint32_t)tmp[(size_t)r * t.ld + c] << 16;
      float f; std::memcpy(&f, &u, 4);
      host_out[(size_t)r * t.C + c] = f;
    }
  NR_CATCH
}
