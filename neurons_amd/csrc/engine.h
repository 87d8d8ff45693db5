// Internal header of the denoiser-network engine behind the C ABI of include/neurons_amd.h: what its translation units share.
//   engine.h            error type and macros, Arena / Act / IO, the WeightStore, the declaration of nr_net
//   engine_weights.hip  the weight store: state dict as loaded, converted device weights, every weight converter, what each fused transformer kernel reads (X_weights)
//   engine_layers.hip   the plan emitters (conv, groupnorm, layernorm, attention, one X_block per fused transformer kernel) and the module builders up to temporal_module
//   engine_nets.hip     the network builders (U-Net / SparseCtrl, sgm U-Net, VAE decoder / encoder, CLIP, leaf modules) and plan()
//   engine_ops.hip      the single-op test hooks (nr_op_*)
//   engine.hip          graph-replay runtime, the C ABI, the engine's two small kernels
//   sampler.hip         the per-step sampler arithmetic behind nr_cfg_* / nr_edm_* / nr_prior_p_sample_step: not the engine, shares its error type and macros
// A plan idiom that is needed twice lives in ONE helper here (WeightStore::packed / convert / stacked / w_temb_projection, nr_net::begin_plan / stage_context /
// context_kv / linear_wb / splitk_scratch / stem / head / downsample_conv / time_embedding / frame_gather, descf); a derived weight name is spelled in engine_weights.hip only; a host-side change of these files is accepted on tools/plan_equal.sh.
#pragma once
#include "launchers.h"
#include "../../include/neurons_amd.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace nre {

void set_err(const std::string& s);      // the text nr_last_error() returns on this thread (engine.hip)

struct NrError : std::runtime_error {
  nr_status code;
  NrError(nr_status c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIP_OK(expr)                                                                                        \
  do {                                                                                                      \
    hipError_t _e = (expr);                                                                                 \
    if (_e != hipSuccess) throw nre::NrError(NR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// launcher return code (unsupported shape) AND the HIP launch status: a rejected launch (bad LDS size, bad grid) must
// fail loudly instead of leaving the previous contents of the output buffer in place
#define LAUNCH_OK(expr)                                                                                   \
  do {                                                                                                    \
    int _r = (expr);                                                                                      \
    if (_r != 0) throw nre::NrError(NR_ERR_UNSUPPORTED, std::string(#expr) + " -> " + std::to_string(_r)); \
    hipError_t _le = hipGetLastError();                                                                   \
    if (_le != hipSuccess) throw nre::NrError(NR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_le)); \
  } while (0)

// body of an extern "C" entry point that returns nr_status
#define NR_TRY try {
#define NR_CATCH                                                                   \
  }                                                                                \
  catch (const nre::NrError& e) { nre::set_err(e.what()); return e.code; }         \
  catch (const std::exception& e) { nre::set_err(e.what()); return NR_ERR_STATE; } \
  return NR_OK;

inline float bf2f_host(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
inline uint16_t f2bf_host(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;  // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// Phase-form weights of a nearest-2x upsample + 3x3 conv (NrGemmParams::ups == 2) from its fp32 taps w[o][c][k] at w[o * so + c * sc + k * sk], k = 3 ky + kx:
// out[((2 py + px) * Cout + o) * 4 + (2 a + b)][c] = bf16( sum_{ky in R(py, a)} sum_{kx in R(px, b)} w[o][c][3 ky + kx] ), R(0,0) = {0}, R(0,1) = {1, 2},
// R(1,0) = {0, 1}, R(1,1) = {2}: the taps of output pixel (2 y + py, 2 x + px) that read source pixel (y + a + py - 1, x + b + px - 1).  Summed in fp32 in
// the order (ky, kx) ascending, rounded once.  The one implementation: the engine's converter and the C ABI both call it
inline void nr_ups_phase_pack(const float* w, size_t so, size_t sc, size_t sk, int Cout, int Cin, uint16_t* out) {
  static const int lo[2][2] = {{0, 1}, {0, 2}}, hi[2][2] = {{0, 2}, {1, 2}};      // R(p, a) = [lo[p][a], hi[p][a]]
  for (int ph = 0; ph < 4; ++ph)
    for (int o = 0; o < Cout; ++o)
      for (int t = 0; t < 4; ++t) {
        const int py = ph >> 1, px = ph & 1, a = t >> 1, b = t & 1;
        uint16_t* dst = out + (((size_t)ph * Cout + o) * 4 + t) * Cin;
        for (int c = 0; c < Cin; ++c) {
          float acc = 0.f;
          for (int ky = lo[py][a]; ky <= hi[py][a]; ++ky)
            for (int kx = lo[px][b]; kx <= hi[px][b]; ++kx) acc += w[o * so + c * sc + (size_t)(3 * ky + kx) * sk];
          dst[c] = f2bf_host(acc);
        }
      }
}

template <class... A>      // an op description: printf into a string (160 characters at the most)
std::string descf(const char* fmt, A... a) { char d[160]; snprintf(d, sizeof(d), fmt, a...); return d; }
// environment switches: "=1 turns it on" and "on unless =0"
inline bool env_is_1(const char* name) {
  const char* v = getenv(name);
  return v && v[0] == '1';
}

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
  int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

// ---- plan-time arena allocator (offsets only; first fit with coalescing) ----
struct Arena {
  struct Blk { size_t off, size; };
  std::vector<Blk> free_;
  size_t top = 0, high = 0;
  static size_t align(size_t b) { return (b + 255) & ~(size_t)255; }
  size_t alloc(size_t bytes);
  void release(size_t off, size_t bytes);
  void reset() { free_.clear(); top = 0; high = 0; }
};

struct Buf {
  Arena* arena; size_t off, bytes; bool keep;
  ~Buf() { if (!keep) arena->release(off, bytes); }
};

// channels-last activation [nimg][H][W][C] (row stride ld elements)
struct Act {
  std::shared_ptr<Buf> buf;
  bf16* ptr = nullptr;
  int nimg = 0, H = 0, W = 0, C = 0, ld = 0;
  int64_t rows() const { return (int64_t)nimg * H * W; }
  bool valid() const { return nimg > 0; }
};

struct Tap { std::string name; bf16* ptr; int64_t rows; int C, ld; };

struct IO {
  const float* sample;
  const float* ctx;
  float* out;
  const void* down_res[16];
  const void* mid_res;
  int has_res;
  const float* cond;
  const float* mask;
  int cond_batch;
  float scale;
  void* out_down[16];
  void* out_mid;
  const float* y;               // sgm "vector" conditioning
  float in_scale;               // sgm c_in; VAE: 1 / scale_factor
  const int* ids;               // CLIP text encoder: token ids [batch][L]
  float in_shift;               // VAE encoder: x * in_scale + in_shift fused into conv_in
  float out_mul, out_add;       // VAE: image post-scaling fused into conv_out
  int clamp01;
  bool operator==(const IO& o) const { return std::memcmp(this, &o, sizeof(IO)) == 0; }
};
// The IO every forward entry point starts from: all bytes zero (padding too: operator== is a memcmp and IO is the graph-cache key) and the
// defaults the networks share, so one set of pointers gives one key whichever entry point it came through
inline IO new_io() {
  IO io;
  std::memset(&io, 0, sizeof(io));
  io.scale = 1.f; io.in_scale = 1.f; io.out_mul = 1.f; io.cond_batch = 1;
  return io;
}

constexpr int NR_MAX_BATCH = 64;   // samples per evaluation (CFG-expanded; the grouped SparseCtrl schedule runs G x 2B of them)

// engine.hip (its kernels stay in that file): dst = src, nbytes a multiple of 16 (debug snapshots only)
void launch_copy16(const void* src, void* dst, size_t nbytes, hipStream_t s);

struct TembSlot { std::string prefix; int off, C; };      // the slice of the batched time-embedding projection that belongs to one ResBlock

// sinusoidal position table [max_len][C] (motion_module.py:225-239), fp32 throughout
std::vector<float> sinusoid_table(int max_len, int C);

// ---- the weights of one handle: the state dict as loaded (host fp32, reference key names) and the converted device weights by derived name
// ("<tag>:<key>" or "<tag>:<key>|<key>|..."; the names are part of the exported manifest).  dry: the planner's sizing pass, in which a converter
// checks shapes and returns null ----
struct WeightStore {
  const bool& dry;
  explicit WeightStore(const bool& sizing_pass) : dry(sizing_pass) {}
  ~WeightStore();
  WeightStore(const WeightStore&) = delete;

  std::map<std::string, HostTensor> host;
  struct DevW { void* ptr; size_t bytes; };
  std::map<std::string, DevW> dev;   // converted weights by derived name: changed only by adopt() / erase()
  size_t weight_bytes = 0;           // sum of dev[].bytes (what is resident)
  // converted weights received from another handle (import_weights): ONE device allocation, dev[] points into it
  char* import_base = nullptr;
  size_t import_bytes = 0;
  bool in_import(const void* p) const { return import_base && (const char*)p >= import_base && (const char*)p < import_base + import_bytes; }

  // ---- the state dict ----
  // nr_net_load_tensor: returns true if converted weights derived from this key were dropped (the handle needs a new plan)
  bool load_tensor(const std::string& key, const float* data, const int64_t* shape, int ndim);
  void release_host();               // nr_net_release_host_weights: the fp32 copies go, the shapes stay
  const HostTensor& need(const std::string& key) const;
  bool has(const std::string& key) const { return host.count(key) != 0; }
  const HostTensor& data_of(const std::string& key) const;      // as need(), and the host copy must still be there
  void check_shape(const std::string& key, const HostTensor& t, std::initializer_list<int64_t> want) const;

  // ---- converted-weight exchange between handles (rank 0 converts once, the bf16 arena travels device to device) ----
  std::string manifest(int kind, size_t* total) const;
  void export_to(void* dst_dev, hipStream_t s) const;            // every converted buffer at its manifest offset
  void import_from(int kind, const std::string& manifest, const void* src_dev, int64_t arena_bytes, hipStream_t s);

  // ---- the converted weights ----
  void* upload(const std::string& name, const void* data, size_t bytes);
  void* adopt(const std::string& name, void* d, size_t bytes);   // the only place that inserts a converted buffer and adds it to the resident total
  void erase(const std::string& name);                           // the only place that removes one
  std::string name_of(const void* p, const char* who) const;     // derived name of the converted matrix this pointer is
  template <class Fn>
  void* cached(const std::string& name, Fn make) {
    if (dry) return nullptr;
    auto it = dev.find(name);
    if (it != dev.end()) return it->second.ptr;
    return make();
  }
  // A buffer a pack kernel fills on the device: fn(d) enqueues the kernel(s) on the null stream, which have run when this returns.  inputs: converted
  // matrices that are ONLY this pack's inputs (a fused kernel's weight stream: its launch never reads them), converted by fn.  Once the buffer exists, the
  // inputs this call had to make are erased again: they neither stay resident nor travel in the exported arena.  An input another plan had already made stays.
  template <class Fn>
  void* packed(const std::string& name, size_t bytes, Fn fn, const std::vector<std::string>& inputs = {}) {
    return cached(name, [&]() {
      std::vector<char> had;
      for (auto& in : inputs) had.push_back(dev.count(in) != 0);
      void* d = nullptr;
      HIP_OK(hipMalloc(&d, bytes));
      try { fn(d); HIP_OK(hipDeviceSynchronize()); }
      catch (...) { (void)hipFree(d); throw; }
      adopt(name, d, bytes);
      for (size_t i = 0; i < inputs.size(); ++i) if (!had[i]) erase(inputs[i]);
      return d;
    });
  }
  // The skeleton of a one-tensor converter: shape check, then (unless cached or sizing) fill(source fp32 data, `count` zeroed elements of T) and
  // upload as "<tag><key>"
  template <class T, class Fill>
  const T* convert(const char* tag, const std::string& key, std::initializer_list<int64_t> shape, size_t count, Fill fill) {
    check_shape(key, need(key), shape);
    const std::string name = tag + key;
    return (const T*)cached(name, [&]() {
      const HostTensor& t = data_of(key);
      std::vector<T> h(count);
      fill(t.data.data(), h.data());
      return upload(name, h.data(), h.size() * sizeof(T));
    });
  }
  // the data of several tensors one after another, each element through cvt (shapes are the caller's to check)
  template <class T, class Cvt>
  const T* stacked(const std::string& name, const std::vector<std::string>& keys, Cvt cvt) {
    return (const T*)cached(name, [&]() {
      std::vector<T> h;
      for (auto& k : keys) { const HostTensor& t = data_of(k); for (float f : t.data) h.push_back(cvt(f)); }
      return upload(name, h.data(), h.size() * sizeof(T));
    });
  }

  // ---- converters (engine_weights.hip) ----
  const bf16* w_linear(const std::string& key, int N, int K);                                       // "lin:"   nn.Linear / 1x1 conv [N][K] -> bf16
  const bf16* w_linear_cat(const std::vector<std::string>& keys, int Neach, int K);                 // "cat:"   rows of several [Neach][K] (fused q|k|v, k|v)
  const float* b_cat(const std::vector<std::string>& keys, int Neach);                              // "bcat:"
  struct Stacked { const bf16* w; const float* b; };
  Stacked w_temb_projection(const std::string& tag, const std::vector<TembSlot>& slots, const std::string& layer, int K);   // "tembw:<tag>" "tembb:<tag>"
  struct LnW { const bf16* w; const float* c; const float* b; };
  LnW w_ln_linear(const std::vector<std::string>& wkeys, const std::vector<std::string>& bkeys, const std::string& ln, int Neach, int K, bool geglu);   // "lnw:" "lnc:" "lnb:"
  const float* pe_projection(const std::vector<std::string>& wkeys, int Neach, int K, int max_len); // "perv:"
  struct FoldW { const bf16* w; const float* b; };
  FoldW w_fold_ff_proj(const std::string& ff2, const std::string& po, int C);                       // "foldw:" "foldb:"
  const bf16* w_geglu(const std::string& key, int inner, int K);                                    // "geglu:"
  const float* b_geglu(const std::string& key, int inner);                                          // "geglub:"
  const bf16* w_conv3(const std::string& key, int Cout, int Cin, bool tap_inner = false);           // "conv3:" / "conv3t:"
  const bf16* w_conv3_ups_phase(const std::string& key, int Cout, int Cin);                         // "conv3up:"  [4 phases][Cout][4 taps][Cin], the taps summed in fp32
  const float* w_conv_in(const std::string& key, int Cout, int Cin);                                // "convin:"
  const bf16* w_condembed(const std::string& key, int Cout, int Cin);                               // "cefm:"
  const float* w_f32_sum(const std::string& a, const std::string& b, int64_t n);                    // "f32sum:"
  const float* w_f32(const std::string& key, std::initializer_list<int64_t> shape);                 // "f32:"   the tensor as it is
  const float* w_f32(const std::string& key, int64_t n) { return w_f32(key, {n}); }
  const float* pe_table(int C, int max_len);                                                        // "pe:"
  const float* b_ln_pe(const std::string& ln, int F, int C);                                        // "tagb:"
  const bf16* w_layout(const bf16* w, int N, int K, int layout);                                    // "fm:" / "w8:" / "l160:" / "l128:<name of w>" (NrWeightLayout)

  // ---- what each fused transformer kernel reads (engine_weights.hip): its packed weight stream [+ epilogue table] and its fp32 vectors.  The shape checks, the
  // stream's derived name, the pack and the converted matrices that only fed it (dropped again: the inputs of packed) live there, beside the converters they name ----
  struct FfFusedW { const bf16* stream; const float *gamma, *beta, *b1, *bc; };
  FfFusedW ff_fused_weights(const std::string& ln, const std::string& ff, const std::string& po, int C);                // "ffs:"   ln: LayerNorm, ff: FeedForward, po: proj_out
  struct XattnFusedW { const bf16* wstream; const float *gamma, *beta, *bo; };
  XattnFusedW xattn_fused_weights(const std::string& b, int C);                                                         // "xas:"   b: the transformer block
  struct TattnFusedW { const bf16* stream; const float *gb, *gamma, *bo; };
  TattnFusedW tattn_fused_weights(const std::string& ln, const std::string& ab, int F, int C);                          // "tas:"   ab: the attention block
  struct HeadW { const bf16* stream; const float* table; };
  HeadW xattn_head_weights(const std::string& ln, const std::string& wq, int C);                                        // "xaws:" "xawt:"
  HeadW tattn_head_weights(const std::string& ln, const std::vector<std::string>& wqkv, int C, int F, int max_len);     // "taws:" "tawe:<max_len>:<F>:"
  LnW ln_vectors(const std::vector<std::string>& wkeys, const std::string& ln, int Neach, int K);      // c / b' of a LayerNorm fold whose matrix may be gone (it fed a stream)
  const float* fold_bias(const std::string& ff2, const std::string& po, int C);                       // bc of a FeedForward fold, likewise
};

}  // namespace nre

struct nr_net {
  using Arena = nre::Arena;
  using Buf = nre::Buf;
  using Act = nre::Act;
  using IO = nre::IO;
  static constexpr int NR_MAX_BATCH = nre::NR_MAX_BATCH;

  nr_net_config cfg;
  int device = -1;                   // HIP device the handle was created on

  // plan
  int B2 = 0, F = 0, H = 0, W = 0, ctx_len = 0;
  bool planned = false;
  bool dry = false;
  nre::WeightStore wts{dry};
  Arena arena;
  // buffers written by the context ops live in their OWN region behind the main arena: context ops execute before
  // everything else, so they must never share memory with any temporary of the main plan
  Arena parena;
  size_t main_high = 0;          // bytes of the main region (known after the sizing pass)
  char* arena_base = nullptr;
  size_t arena_bytes = 0;
  std::vector<std::function<void(hipStream_t)>> ops;
  // ops that depend only on the cross-attention context (fp32->bf16 convert + every to_k|to_v projection): the
  // context is constant over all denoising steps of a clip, so they run once per context (nr_net_invalidate_context)
  std::vector<std::function<void(hipStream_t)>> ctx_ops;
  std::vector<Act> ctx_persist;      // K|V buffers that must survive between forwards
  bool building_ctx = false;
  bool ctx_dirty = true;
  struct OpMeta { int kind; double flops, bytes; std::string desc; int launches = 1; };   // launches: kernels this op enqueues
  std::vector<OpMeta> op_meta;   // parallel to ops: kernel class + algorithmic work (for roofline reporting)
  std::vector<nre::Tap> taps;
  bool keep_all = false;
  // nr_net_set_deterministic_batch / NR_DETERMINISTIC_BATCH=1: every plan choice that can move a rounding point or a summation order (LayerNorm
  // folded vs separate, split-K depth, row-panel / fused-kernel eligibility, GroupNorm variant and chunking, the weight-stream rotation of
  // the fused kernels) is made for the rows of ONE clip's CFG pair, so a clip's result does not depend on how many clips share the call
  bool det_batch = false;
  int clip_samples = 2;          // nr_net_set_clip_samples: samples of ONE clip in the batch (2 = CFG pair, 1 = no guidance)
  long long det_rows(long long rows) const {       // rows of this op that belong to one clip (rows itself when not in that mode)
    if (!det_batch || B2 <= clip_samples) return rows;
    return rows / B2 * clip_samples;
  }
  // SparseCtrl only (nr_sparsectrl_set_condition_frames): the frames whose condition / mask is not all zero.  With the noisy sample zeroed
  // (sparse_controlnet.py:468-469) every OTHER frame enters the network as the same constant image (conv_in(0) + cond_embedding(0) =
  // the two biases, :513-521), so until the first motion module mixes frames (unet_blocks.py:382-421: resnet -> attention -> motion
  // module) all of them carry identical activations: down_blocks[0].resnets[0] + attentions[0] run on the conditioned frames plus ONE
  // representative of the rest and are broadcast before motion_modules[0].  Exact (per-frame operators, identical inputs); < 0 = off.
  int n_cond_frames = -1;
  int cond_frames[64] = {0};
  bool cfg_dup = false;          // nr_net_set_cfg_pair_identical: the caller promises sample[b] == sample[b + B2/2] and timestep[b] == timestep[b + B2/2]
  bool attn_fp8 = false;         // nr_net_set_attention_fp8: spatial / cross attention on e4m3 MFMA operands (config 5)
  int ups_phase_mode = -1;       // NR_UPS_PHASE as read when the plan began (begin_plan): 0 never the phase form, 1 every eligible upsample conv, -1 (unset) nr_ups_phase_rule
  bool w8 = false;               // nr_net_set_weight_fp8 (new handles: NR_W8=1): the Linears smallm.hip serves read their checkpoint matrices as e4m3 codes
                                 // with one power-of-two scale per row (NrGemmParams::w8); a numerics variant, bf16 is the default
  IO io = nre::new_io();
  int n_res = 0;
  struct ResShape { int C, h, w; };
  std::vector<ResShape> res_shapes;  // n_res down + 1 mid

  // small persistent fp32 buffers (allocated from the arena, pinned)
  float* t_dev = nullptr;
  int temb_total = 0;

  // graph
  bool use_graph = false;
  // [0] ops before the ControlNet-residual adds, [1] the adds, [2] the rest
  // captured graphs per segment, keyed by the IO block they were captured with (pointers are baked into the kernel nodes): the grouped
  // SparseCtrl schedule alternates between a few residual-buffer sets, each gets its own executable graph (small LRU)
  struct GraphSlot { IO io = nre::new_io(); hipGraphExec_t exec = nullptr; unsigned long long used = 0; };
  static constexpr int NR_GRAPH_SLOTS = 64;     // the sgm Euler loop bakes c_in(sigma) into its graphs: one per step of a 38 / 50-step schedule
  std::vector<GraphSlot> gcache[3];
  unsigned long long gclock = 0;
  hipEvent_t ev_slot[2] = {nullptr, nullptr};   // completion of nr_sparsectrl_forward_async evaluations (two in flight at most)
  size_t split_op = 0;                            // index of the first op of segment 1 (== ops.size() if none)
  size_t split_op2 = 0;                           // index of the first op of segment 2
  hipEvent_t ev_adds = nullptr;                   // U-Net: the residual adds have consumed SparseCtrl's outputs
  // SparseCtrl evaluation issued ahead of time for the NEXT denoising step (nr_denoise_step_forward): its inputs do
  // not depend on the latents, only on the timestep / context / condition
  bool prefetch_valid = false;
  float prefetch_t[NR_MAX_BATCH] = {0};
  IO prefetch_io = nre::new_io();
  // graph replay happens on an engine-owned non-blocking stream (capture is illegal on the legacy default
  // stream PyTorch hands over); it is fenced to the caller's stream with two events per forward
  hipStream_t own_stream = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;

  ~nr_net();

  // ------------------------------------------------------------------ plan helpers
  // (integer arithmetic: during the sizing pass arena_base is null and the pointers are never used; `null + offset` on a pointer is UB)
  template <class T>
  T* at(size_t off) const { return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(arena_base) + off); }
  Act new_act(int nimg, int h, int w, int C) { return act_in(arena, 0, keep_all, nimg, h, w, C); }
  Act new_act_persistent(int nimg, int h, int w, int C) { return act_in(parena, main_high, true, nimg, h, w, C); }
  Act act_in(Arena& a, size_t base, bool keep, int nimg, int h, int w, int C);
  // raw pinned scratch (lives for the whole plan)
  template <class T>
  T* new_scratch(size_t count) { return at<T>(arena.alloc(count * sizeof(T))); }
  // temporary fp32 scratch with lifetime of the returned handle
  std::shared_ptr<Buf> new_tmp(size_t bytes);
  // split-K slabs of an igemm (NrGemmRoute::ws_bytes; small-M / huge-K layers): scratch with the lifetime of the returned handle, null if none
  struct SplitK { std::shared_ptr<Buf> buf; float* ws = nullptr; };
  SplitK splitk_scratch(size_t bytes);
  void emit(std::function<void(hipStream_t)> fn, int kind = NR_PROF_OTHER, double flops = 0, double bytes = 0, const std::string& desc = std::string());
  void last_op_launches(int n) { if (!dry && !building_ctx && !op_meta.empty()) op_meta.back().launches = n; }
  void tap(const std::string& name, const Act& a) {
    if (!dry && keep_all) taps.push_back(nre::Tap{name, a.ptr, a.rows(), a.C, a.ld});
  }
  void op_tap(const char* kind, const Act& a);      // debug only (NR_OP_TAPS=1 with nr_net_set_debug): one tap per kernel output
  // what every network builder starts with: an empty plan (ops, context ops, taps, both arenas, time-embedding slots, residual shapes; the context
  // ops are due again) and the timestep buffer as the first allocation of the arena
  void begin_plan();
  Act stage_context();           // the text context fp32 -> bf16 [B2 * ctx_len][cross_dim], as a context op
  // K | V of the text context for the cross-attention of transformer block b: a persistent [.., 2C] activation written by a context op (run again
  // only when the context changes).  pack(kv, ldkv, stream, s): a further context op that re-arranges K | V for a fused kernel into a persistent stream
  // of stream_bytes; the stream is returned instead
  Act context_kv(const Act& ctx_bf, const std::string& b, int C, size_t stream_bytes = 0, const std::function<void(const bf16*, int, bf16*, hipStream_t)>& pack = nullptr);

  // ------------------------------------------------------------------ emitters and module builders (engine_layers.hip)
  struct GemmOpt {
    const float* bias = nullptr;
    const float* rowvec = nullptr; int rowvec_div = 1, rowvec_ld = 0, rowvec_mod = 0;
    const Act* res = nullptr;
    float scale = 1.f;
    int geglu = 0;
    Act* out = nullptr;      // write into this existing activation (may alias res)
    int pad_tl0 = 0;         // 3x3: no top/left padding (VAE Downsample)
    int act = 0;             // 1: quick_gelu
    const float* ln_c = nullptr;   // LayerNorm folded into this GEMM (see w_ln_linear)
    int tap_inner = 0;       // 3x3 stride 1 single source: weights in the tap-inner layout of w_conv3(.., tap_inner)
    bool derived_w = false;  // w is a product the engine computed (w_fold_ff_proj), not a checkpoint tensor: it stays bf16 under nr_net_set_weight_fp8
  };
  Act conv(const Act& x0, const Act* x1, const bf16* w, int Cout, int ksize, int stride, int ups, const GemmOpt& o);
  Act linear(const Act& x, const bf16* w, int N, const GemmOpt& o) { return conv(x, nullptr, w, N, 1, 1, 0, o); }
  // nearest-2x upsample + 3x3 conv `wkey` ([Cout][x.C][3][3]): on the replicated image (ups = 1, w_conv3) or as four 2x2 phase convs on the source
  // (ups = 2, w_conv3_ups_phase), decided here once per plan (ups_phase_mode); the layer keeps only the weight form it runs with
  Act upsample_conv(const Act& x, const std::string& wkey, int Cout, const GemmOpt& o);
  Act linear_wb(const Act& x, const std::string& key, int N, const Act* res = nullptr, Act* out = nullptr);      // linear() with <key>.weight / <key>.bias
  void gemm_raw(const bf16* a, int lda, const bf16* w, int M, int N, int K, const float* bias, bf16* out, int ldo, float* out32, const char* what);
  Act groupnorm(const Act& x0, const Act* x1, const std::string& prefix, float eps, int silu);
  Act layernorm(const Act& x, const std::string& prefix, const float* pe, int pe_F);
  Act attention(int mode, const Act& q, const Act* kv, int C, int heads, int causal = 0);
  using TembSlot = nre::TembSlot;
  std::vector<TembSlot> temb_slots;   // add_temb_slot: one per ResBlock, before time_embedding
  float* temb_all = nullptr;          // [B2][temb_total]
  const float* temb_for(const std::string& prefix, int C);
  struct ResKeys { std::string norm1, conv1, norm2, conv2, shortcut; };
  ResKeys res_keys(const std::string& pre) const;
  Act resnet(const Act& x0, const Act* x1, const std::string& pre, int Cout);
  Act ln_linear(const Act& x, const std::string& ln, const std::vector<std::string>& wkeys, const std::vector<std::string>& bkeys, int Neach, bool geglu,
                int act, bool temporal_pe);
  void feed_forward(Act& t, const std::string& ln, const std::string& pre);
  Act feed_forward_proj_out(const Act& x, Act& t, const std::string& ln, const std::string& ff, const std::string& pre);
  bool cfg_dedup_active() const;
  Act expand_cfg(const Act& h);
  enum BlockKernel { BLOCK_UNFUSED, BLOCK_FUSED320, BLOCK_HEAD };      // a cross- / temporal-attention block on t: GEMMs + attention, the fused C = 320 kernel, the head kernel above it
  BlockKernel cross_attn_kernel(const Act& t, int heads, int hw) const;
  BlockKernel temporal_attn_kernel(const Act& t, int heads, int hw) const;
  Act ff_fused_block(const Act& x, const Act& t, const std::string& ln, const std::string& ff, const std::string& po);      // -> out
  void xattn_fused_block(Act& t, const Act& ctx_bf, const std::string& b, int hw);                                            // t in place
  Act xattn_head_block(const Act& t, const Act& ctx_bf, const std::string& b, int hw);                                        // -> a, before to_out
  void tattn_fused_block(Act& t, const std::string& nrm, const std::string& ab, int hw, int heads);                          // t in place
  Act tattn_head_block(const Act& t, const std::string& nrm, const std::vector<std::string>& wqkv, int hw, int heads);       // -> a, before to_out
  Act spatial_transformer(const Act& x_in, const Act& ctx_bf, const std::string& pre, int depth = 1, bool cfg_half = false, Act* x_full = nullptr);
  Act temporal_module(const Act& x, const std::string& pre0);
  Act vae_attn(const Act& x, const std::string& pre);

  // ------------------------------------------------------------------ networks (engine_nets.hip)
  // emitters the builders share.  What the 4-channel stem reads is resolved when the op launches: io.sample (`batch` samples; affine: x * io.in_scale + io.in_shift),
  // io.cond + io.mask (C + 1 planes of io.cond_batch condition images), or a plan-time buffer such as the VAE decoder's post_quant output
  struct StemIn { enum { SAMPLE, COND, BUFFER } from; int C, batch; const float* buf = nullptr; bool affine = false; };
  std::function<void(hipStream_t)> stem(const StemIn& in, const std::string& key, const Act& out, const char* addend_key = nullptr);
  void head(const Act& x, const std::string& norm, const std::string& conv, int Cout, const char* quant = nullptr);
  Act downsample_conv(const Act& x, const std::string& key, const std::string& tap_name, int pad_tl0 = 0);
  void add_temb_slot(const std::string& prefix, int C) { temb_slots.push_back(TembSlot{prefix, temb_total, C}); temb_total += C; }
  void time_embedding(const std::string& l1, const std::string& l2, const char* label, const std::string& tag, const std::string& layer);
  // the identical-frame evaluation (n_cond_frames): the n distinct frames to evaluate and, per frame, which of them it equals; empty = off
  struct FrameDedup { std::vector<int> reduce, expand; int n() const { return (int)reduce.size(); } };
  FrameDedup identical_frames() const;
  Act frame_gather(const Act& x, int Fs, const std::vector<int>& map);
  Act embed_conv(const Act& in, int Fe, const std::string& key, int Cout, int stride, int silu, const float* bias);
  void cond_embedding(Act& x, const FrameDedup& fd);
  // the builders: one per network kind, each in the order of its reference forward()
  struct Trunk { Act x, ctx; std::vector<Act> skips; };      // mid-block output, bf16 text context, the n_res down-block residuals
  Trunk down_mid();
  void residual_adds(const Trunk& t);
  void build_unet3d();
  void build_sparsectrl();
  struct SgmLayout {
    struct In { int idx; int kind; int level; int Cout; };          // kind 0 conv_in, 1 res(+attn), 2 downsample
    struct Out { int idx; int level; int Cout; bool attn; bool up; };
    std::vector<In> in;
    std::vector<Out> out;
  };
  SgmLayout sgm_layout() const;
  void build_sgm();
  void build_vae();
  void build_vae_enc();
  void build_clip();
  void build_leaf();
  void build();                  // dispatch on cfg.kind
  void plan(int batch, int frames, int h, int w, int ctxl);

  // ------------------------------------------------------------------ runtime (engine.hip)
  void drop_graphs();
  void ensure_streams();
  void run_context(hipStream_t s);           // context-only work (eager, stream-ordered before the main graph); no-op while the context is unchanged
  void set_timesteps(hipStream_t s, const float* timesteps);
  void launch_segment(hipStream_t s, int seg);   // launch the ops of segment `seg` on `s` as a (re)captured hipGraph
  void begin(hipStream_t s, const float* timesteps) { set_timesteps(s, timesteps); run_context(s); }   // what every evaluation starts with on its stream
  void run_eager(hipStream_t s, const float* timesteps);                 // everything in stream order on s
  hipStream_t begin_fenced(hipStream_t caller, const float* timesteps);  // graph mode: the engine's own stream, fenced behind the caller's
  void run(hipStream_t caller, const float* timesteps);
};
