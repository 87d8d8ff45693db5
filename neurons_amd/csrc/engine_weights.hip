// The weight store of an engine handle (engine.h): the state dict as loaded, the converted device weights in the layouts the kernels want
// (bf16, tap-major conv weights, fused q|k|v, GEGLU value/gate interleave, LayerNorm folds, packed weight streams), the manifest they travel
// between handles with, every converter and the weight bundle of each fused transformer kernel.  Host code only.
#include "engine.h"

namespace nre {

std::vector<float> sinusoid_table(int max_len, int C) {
  std::vector<float> h((size_t)max_len * C);
  const float k = (float)(-std::log(10000.0) / (double)C);
  for (int pos = 0; pos < max_len; ++pos)
    for (int i = 0; i < C; i += 2) {
      const float a = (float)pos * std::exp((float)i * k);
      h[(size_t)pos * C + i] = std::sin(a);
      if (i + 1 < C) h[(size_t)pos * C + i + 1] = std::cos(a);
    }
  return h;
}

// GEGLU row order of the kernels: each 32-row group is 16 value rows, then their 16 gate rows.  Source row of output row n of a
// [2 * inner][K] projection (value rows [0, inner), gate rows [inner, 2 * inner))
static int geglu_src_row(int n, int inner) {
  const int q = n / 32, j = n % 32;
  return j < 16 ? q * 16 + j : inner + q * 16 + (j - 16);
}

// Derived names that a second place needs (the fused kernels' weight bundles at the end of this file name the matrices their streams are packed from):
// spelled here only.  The one-tensor converters' are <tag><key>; part: 'w' the matrix, 'c' / 'b' its fp32 vectors
static const char* const TAG_LIN = "lin:";
static const char* const TAG_GEGLU = "geglu:";
static std::string ln_name(char part, const std::vector<std::string>& wkeys, const std::vector<std::string>& bkeys, const std::string& ln) {      // "lnw:" "lnc:" "lnb:"
  std::string name = std::string("ln") + part + ":" + ln + "|";
  for (auto& k : wkeys) name += k + "|";
  for (auto& k : bkeys) name += k + "|";
  return name;
}
static std::string fold_name(char part, const std::string& ff2, const std::string& po) {      // "foldw:" "foldb:"
  return std::string("fold") + part + ":" + po + ".weight|" + po + ".bias|" + ff2 + ".weight|" + ff2 + ".bias";
}

WeightStore::~WeightStore() {
  while (!dev.empty()) erase(std::string(dev.begin()->first));
  if (import_base) (void)hipFree(import_base);
}

// ------------------------------------------------------------------ the state dict
const HostTensor& WeightStore::need(const std::string& key) const {
  auto it = host.find(key);
  if (it == host.end()) throw NrError(NR_ERR_MISSING_WEIGHT, "missing state-dict entry: " + key);
  return it->second;
}
// host copies may have been released after the first plan (nr_net_release_host_weights)
const HostTensor& WeightStore::data_of(const std::string& key) const {
  const HostTensor& t = need(key);
  if ((int64_t)t.data.size() != t.numel())
    throw NrError(NR_ERR_STATE, import_base
                                    ? "this handle was filled by nr_net_import_weights (no fp32 host weights) and the requested shape needs a converted "
                                      "weight the exporting plan did not make (" + key + "): export from a handle planned for THIS shape, or load a state dict"
                                    : "host copy of " + key + " was released (nr_net_release_host_weights) and this shape needs a conversion the earlier "
                                      "plans did not make; load the state dict again, or do not release the host copies");
  return t;
}
void WeightStore::check_shape(const std::string& key, const HostTensor& t, std::initializer_list<int64_t> want) const {
  int64_t nw = 1; for (auto s : want) nw *= s;
  if (t.numel() != nw)
    throw NrError(NR_ERR_ARG, "state-dict entry " + key + " has " + std::to_string(t.numel()) + " elements, expected " + std::to_string(nw));
}

bool WeightStore::load_tensor(const std::string& k, const float* data, const int64_t* shape, int ndim) {
  HostTensor t;
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= shape[i]; }
  t.data.assign(data, data + n);
  host[k] = std::move(t);
  // a reload invalidates the converted copies derived from exactly this key.  Converted names are "<tag>:<key>" or
  // "<tag>:<key>|<key>|..." (keys contain neither ':' nor '|'); the stacked time-embedding projections ("temb...") are rebuilt
  // when any time-embedding tensor changes.
  // (the sgm ResBlocks call theirs "<block>.emb_layers.1": openaimodel.py:283-289)
  const bool is_temb_src = k.find("time_emb") != std::string::npos || k.find("label_emb") != std::string::npos ||
                           k.find("emb_layers") != std::string::npos;
  auto derived_from = [&](const std::string& name) {
    size_t b = 0;
    while (b <= name.size()) {
      size_t e = name.find_first_of(":|", b);
      if (e == std::string::npos) e = name.size();
      if (e - b == k.size() && name.compare(b, k.size(), k) == 0) return true;
      // a norm enters a name by its prefix ("lnw:<prefix>|..." uses <prefix>.weight and <prefix>.bias)
      if (e > b && k.size() > e - b && k.compare(0, e - b, name, b, e - b) == 0 && (k.compare(e - b, std::string::npos, ".weight") == 0 ||
                                                                                   k.compare(e - b, std::string::npos, ".bias") == 0)) return true;
      b = e + 1;
    }
    return false;
  };
  std::vector<std::string> stale;
  for (auto& kv : dev) if (derived_from(kv.first) || (is_temb_src && kv.first.rfind("temb", 0) == 0)) stale.push_back(kv.first);
  if (stale.empty()) return false;
  (void)hipDeviceSynchronize();
  for (auto& name : stale) erase(name);      // weight_bytes stays the sum of what is resident
  return true;
}

void WeightStore::release_host() {
  for (auto& kv : host) { std::vector<float>().swap(kv.second.data); }
}

// ------------------------------------------------------------------ manifest, export, import
// Manifest: text, one record per line.  "H <state-dict key> <ndim> <dims...>" for every loaded tensor (shapes only),
// "D <converted name> <offset> <bytes>" for every converted device buffer, offsets 256-byte aligned in name order.
std::string WeightStore::manifest(int kind, size_t* total) const {
  std::string m = "NRW1 " + std::to_string(kind) + "\n";
  for (auto& kv : host) {
    m += "H " + kv.first + " " + std::to_string(kv.second.shape.size());
    for (auto d : kv.second.shape) m += " " + std::to_string(d);
    m += "\n";
  }
  size_t off = 0;
  for (auto& kv : dev) {
    const size_t b = kv.second.bytes;
    m += "D " + kv.first + " " + std::to_string(off) + " " + std::to_string(b) + "\n";
    off += (b + 255) & ~(size_t)255;
  }
  if (total) *total = off;
  return m;
}

void WeightStore::export_to(void* dst_dev, hipStream_t s) const {
  size_t off = 0;
  for (auto& kv : dev) {
    const size_t b = kv.second.bytes;
    HIP_OK(hipMemcpyAsync((char*)dst_dev + off, kv.second.ptr, b, hipMemcpyDeviceToDevice, s));
    off += (b + 255) & ~(size_t)255;
  }
}

void WeightStore::import_from(int kind, const std::string& m, const void* src_dev, int64_t arena_bytes, hipStream_t s) {
  if (!dev.empty() || !host.empty()) throw NrError(NR_ERR_STATE, "import into a fresh handle (no tensors loaded, not planned)");
  size_t pos = 0;
  auto next_line = [&](std::string& line) {
    if (pos >= m.size()) return false;
    const size_t e = m.find('\n', pos);
    line = m.substr(pos, e == std::string::npos ? std::string::npos : e - pos);
    pos = e == std::string::npos ? m.size() : e + 1;
    return true;
  };
  std::string line;
  if (!next_line(line) || line.rfind("NRW1 ", 0) != 0) throw NrError(NR_ERR_ARG, "bad manifest header");
  if (std::atoi(line.c_str() + 5) != kind) throw NrError(NR_ERR_ARG, "manifest is for a different network kind");
  if (arena_bytes <= 0) throw NrError(NR_ERR_ARG, "empty arena");
  // parse and validate the WHOLE manifest into temporaries first: a bad line must leave the handle fresh (importable again)
  std::map<std::string, HostTensor> new_host;
  struct DevRec { std::string name; size_t off, bytes; };
  std::vector<DevRec> new_dev;
  while (next_line(line)) {
    if (line.size() < 3) continue;
    std::vector<std::string> tok;
    size_t a = 0;
    while (a < line.size()) { size_t b = line.find(' ', a); if (b == std::string::npos) b = line.size(); if (b > a) tok.push_back(line.substr(a, b - a)); a = b + 1; }
    if (tok.empty()) continue;
    if (tok[0] == "H" && tok.size() >= 3) {
      HostTensor t;                                   // shape only: the data never exists on this rank
      const int nd = std::atoi(tok[2].c_str());
      if (nd < 0 || nd > 8 || 3 + nd != (int)tok.size()) throw NrError(NR_ERR_ARG, "bad manifest line: " + line);
      for (int i = 0; i < nd; ++i) {
        const long long d = std::atoll(tok[3 + i].c_str());
        if (d < 0) throw NrError(NR_ERR_ARG, "bad manifest line: " + line);
        t.shape.push_back(d);
      }
      new_host[tok[1]] = std::move(t);
    } else if (tok[0] == "D" && tok.size() == 4) {
      const long long off = std::atoll(tok[2].c_str()), b = std::atoll(tok[3].c_str());
      if (off < 0 || b <= 0 || off > arena_bytes || b > arena_bytes - off) throw NrError(NR_ERR_ARG, "manifest entry beyond the arena: " + tok[1]);
      new_dev.push_back(DevRec{tok[1], (size_t)off, (size_t)b});
    } else throw NrError(NR_ERR_ARG, "bad manifest line: " + line);
  }
  char* base = nullptr;
  HIP_OK(hipMalloc((void**)&base, (size_t)arena_bytes));
  if (hipMemcpyAsync(base, src_dev, (size_t)arena_bytes, hipMemcpyDeviceToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
    (void)hipFree(base);
    throw NrError(NR_ERR_HIP, "copying the weight arena failed");
  }
  // commit
  import_base = base;
  import_bytes = (size_t)arena_bytes;
  host = std::move(new_host);
  for (auto& r : new_dev) adopt(r.name, base + r.off, r.bytes);
}

// ------------------------------------------------------------------ the converted weights
void* WeightStore::upload(const std::string& name, const void* data, size_t bytes) {
  void* d = nullptr;
  HIP_OK(hipMalloc(&d, bytes));
  HIP_OK(hipMemcpy(d, data, bytes, hipMemcpyHostToDevice));
  return adopt(name, d, bytes);
}
void* WeightStore::adopt(const std::string& name, void* d, size_t bytes) {
  dev[name] = DevW{d, bytes};
  weight_bytes += bytes;
  return d;
}
// frees it (unless it lies inside the imported arena) and takes it out of the resident total.  Also how a converted buffer that only fed another
// conversion (the packed weight streams of the fused kernels) goes again: it then neither stays resident nor travels in the exported arena
void WeightStore::erase(const std::string& name) {
  auto it = dev.find(name);
  if (it == dev.end()) return;
  if (it->second.ptr && !in_import(it->second.ptr)) (void)hipFree(it->second.ptr);
  weight_bytes -= it->second.bytes;
  dev.erase(it);
}
std::string WeightStore::name_of(const void* p, const char* who) const {
  for (const auto& kv : dev) if (kv.second.ptr == p) return kv.first;
  throw NrError(NR_ERR_STATE, std::string(who) + ": not a converted weight matrix");
}

// a converted [N][K] weight matrix in the layout a GEMM route names (NrWeightLayout): w itself, or its packed copy -- fragment-major (smallm.hip), its
// e4m3 form (codes + row scales), the stage stream of lin160.hip, the 128-column stream of its register-panel form; the row-major matrix stays
// (launches of other row counts use it: the e4m3 form therefore ADDS N K + 4 N bytes per matrix, it saves no memory)
const bf16* WeightStore::w_layout(const bf16* w, int N, int K, int layout) {
  if (layout == NR_W_ROWMAJOR || layout == NR_W_TAP_INNER) return w;
  const size_t nb = nr_gemm_packed_bytes(layout, N, K);
  if (!nb) throw NrError(NR_ERR_STATE, "w_layout: shape has no packed form");
  const char* prefix = layout == NR_W_FRAGMAJOR ? "fm:" : (layout == NR_W_FRAGMAJOR_E4M3 ? "w8:" : (layout == NR_W_LIN128Q ? "l128:" : "l160:"));
  return (const bf16*)packed(prefix + name_of(w, "w_layout"), nb, [&](void* d) { LAUNCH_OK(nr_launch_gemm_w_pack(layout, w, N, K, (bf16*)d, nullptr)); });
}

const bf16* WeightStore::w_linear(const std::string& key, int N, int K) {
  const size_t n = (size_t)N * K;
  return (const bf16*)convert<uint16_t>(TAG_LIN, key, {N, K}, n, [&](const float* s, uint16_t* h) { for (size_t i = 0; i < n; ++i) h[i] = f2bf_host(s[i]); });
}
const bf16* WeightStore::w_linear_cat(const std::vector<std::string>& keys, int Neach, int K) {
  std::string name = "cat:";
  for (auto& k : keys) { check_shape(k, need(k), {Neach, K}); name += k + "|"; }
  return (const bf16*)stacked<uint16_t>(name, keys, f2bf_host);
}
const float* WeightStore::b_cat(const std::vector<std::string>& keys, int Neach) {
  std::string name = "bcat:";
  for (auto& k : keys) { check_shape(k, need(k), {Neach}); name += k + "|"; }
  return stacked<float>(name, keys, [](float f) { return f; });
}
// the time-embedding projections <slot prefix><layer> ([slot C][K] each) of every ResBlock stacked into ONE Linear
WeightStore::Stacked WeightStore::w_temb_projection(const std::string& tag, const std::vector<TembSlot>& slots, const std::string& layer, int K) {
  std::vector<std::string> wk, bk;
  for (auto& sl : slots) {
    wk.push_back(sl.prefix + layer + ".weight"); bk.push_back(sl.prefix + layer + ".bias");
    check_shape(wk.back(), need(wk.back()), {sl.C, K});
    check_shape(bk.back(), need(bk.back()), {sl.C});
  }
  Stacked r;
  r.w = (const bf16*)stacked<uint16_t>("tembw:" + tag, wk, f2bf_host);
  r.b = stacked<float>("tembb:" + tag, bk, [](float f) { return f; });
  return r;
}

// LayerNorm folded into the consuming Linear: y = W (gamma * xhat + beta) + b = rstd * (W' x - mean * c) + b'
// with W'[n][k] = gamma[k] W[n][k] (bf16), c[n] = sum_k W'[n][k], b'[n] = b[n] + sum_k beta[k] W[n][k].
// The igemm accumulates the row statistics of x itself (gemm.hip, LNF), so no LayerNorm pass touches HBM.
// wkeys: matrices [Neach][K] stacked along N (fused q|k|v); bkeys: their biases (empty = none);
// geglu: single [2*Neach][K] projection with the value/gate row interleave of w_geglu.
WeightStore::LnW WeightStore::w_ln_linear(const std::vector<std::string>& wkeys, const std::vector<std::string>& bkeys, const std::string& ln, int Neach,
                                          int K, bool geglu) {
  const int rows_each = geglu ? 2 * Neach : Neach;
  for (auto& k : wkeys) check_shape(k, need(k), {rows_each, K});
  for (auto& k : bkeys) check_shape(k, need(k), {rows_each});
  check_shape(ln + ".weight", need(ln + ".weight"), {K});
  check_shape(ln + ".bias", need(ln + ".bias"), {K});
  LnW r{nullptr, nullptr, nullptr};
  if (dry) return r;
  const std::string nw = ln_name('w', wkeys, bkeys, ln), nc = ln_name('c', wkeys, bkeys, ln), nb = ln_name('b', wkeys, bkeys, ln);
  auto it = dev.find(nw), ic = dev.find(nc), ib = dev.find(nb);
  if (it != dev.end() && ic != dev.end() && ib != dev.end()) return LnW{(const bf16*)it->second.ptr, (const float*)ic->second.ptr, (const float*)ib->second.ptr};
  erase(nw); erase(nc); erase(nb);                                 // partly present (matrix dropped after a stream pack): rebuild all three
  const HostTensor& g = data_of(ln + ".weight");
  const HostTensor& be = data_of(ln + ".bias");
  const size_t N = (size_t)rows_each * wkeys.size();
  std::vector<uint16_t> hw(N * K);
  std::vector<float> hc(N), hb(N);
  for (size_t mi = 0; mi < wkeys.size(); ++mi) {
    const HostTensor& W = data_of(wkeys[mi]);
    const HostTensor* B = bkeys.empty() ? nullptr : &data_of(bkeys[mi]);
    for (int n = 0; n < rows_each; ++n) {
      const int src = geglu ? geglu_src_row(n, Neach) : n;
      const float* wr = W.data.data() + (size_t)src * K;
      const size_t dst = mi * rows_each + n;
      double c = 0.0, b = B ? (double)B->data[src] : 0.0;
      for (int k = 0; k < K; ++k) {
        const uint16_t q16 = f2bf_host(g.data[k] * wr[k]);
        hw[dst * K + k] = q16;
        c += (double)bf2f_host(q16);
        b += (double)be.data[k] * (double)wr[k];
      }
      hc[dst] = (float)c; hb[dst] = (float)b;
    }
  }
  r.w = (const bf16*)upload(nw, hw.data(), hw.size() * 2);
  r.c = (const float*)upload(nc, hc.data(), hc.size() * 4);
  r.b = (const float*)upload(nb, hb.data(), hb.size() * 4);
  return r;
}
// temporal positional encoding pushed through the q|k|v projection: rv[f][n] = sum_k pe[f][k] W[n][k], f < max_len
// (motion_module.py:241-243,274-278 add pe AFTER the LayerNorm, so W(LN(x) + pe) = W LN(x) + W pe)
const float* WeightStore::pe_projection(const std::vector<std::string>& wkeys, int Neach, int K, int max_len) {
  std::string name = "perv:" + std::to_string(max_len) + ":";
  for (auto& k : wkeys) name += k + "|";
  return (const float*)cached(name, [&]() {
    const size_t N = (size_t)Neach * wkeys.size();
    const std::vector<float> pe = sinusoid_table(max_len, K);
    std::vector<float> rv((size_t)max_len * N);
    for (size_t mi = 0; mi < wkeys.size(); ++mi) {
      const HostTensor& W = data_of(wkeys[mi]);
      for (int n = 0; n < Neach; ++n)
        for (int f = 0; f < max_len; ++f) {
          double a = 0.0;
          const float* wr = W.data.data() + (size_t)n * K;
          const float* pr = pe.data() + (size_t)f * K;
          for (int k = 0; k < K; ++k) a += (double)pr[k] * (double)wr[k];
          rv[(size_t)f * N + mi * Neach + n] = (float)a;
        }
    }
    return upload(name, rv.data(), rv.size() * 4);
  });
}
// FeedForward.net.2 followed by proj_out (only the residual add of the block between them) folded into one Linear over the
// concatenated operand [t | g]: Wc = [Wpo | Wpo Wff2] ([C][5C] bf16), bc = bpo + Wpo bff2.  The C x C x 4C product runs on the device
// in fp32 (fold_linear_pair_kernel), once per plan of new weights.
WeightStore::FoldW WeightStore::w_fold_ff_proj(const std::string& ff2, const std::string& po, int C) {
  const int J = 4 * C;
  check_shape(ff2 + ".weight", need(ff2 + ".weight"), {C, J});
  check_shape(ff2 + ".bias", need(ff2 + ".bias"), {C});
  check_shape(po + ".weight", need(po + ".weight"), {C, C});
  check_shape(po + ".bias", need(po + ".bias"), {C});
  FoldW r{nullptr, nullptr};
  if (dry) return r;
  const std::string nw = fold_name('w', ff2, po), nb = fold_name('b', ff2, po);
  auto it = dev.find(nw), itb = dev.find(nb);
  if (it != dev.end() && itb != dev.end()) return FoldW{(const bf16*)it->second.ptr, (const float*)itb->second.ptr};
  if (itb != dev.end()) erase(nb);                                 // bias kept, matrix dropped after a stream pack: rebuild both
  const HostTensor& W2 = data_of(po + ".weight");
  const HostTensor& B2 = data_of(po + ".bias");
  const HostTensor& W1 = data_of(ff2 + ".weight");
  const HostTensor& B1 = data_of(ff2 + ".bias");
  const size_t wcb = (size_t)C * (C + J) * sizeof(bf16), bcb = (size_t)C * sizeof(float);
  r.w = (const bf16*)packed(nw, wcb, [&](void* dwc) {
    float *dw2 = nullptr, *dw1 = nullptr, *db2 = nullptr, *db1 = nullptr;
    void* dbc = nullptr;
    HIP_OK(hipMalloc(&dw2, W2.data.size() * 4)); HIP_OK(hipMalloc(&dw1, W1.data.size() * 4));
    HIP_OK(hipMalloc(&db2, B2.data.size() * 4)); HIP_OK(hipMalloc(&db1, B1.data.size() * 4));
    HIP_OK(hipMalloc(&dbc, bcb));
    HIP_OK(hipMemcpy(dw2, W2.data.data(), W2.data.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dw1, W1.data.data(), W1.data.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(db2, B2.data.data(), B2.data.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(db1, B1.data.data(), B1.data.size() * 4, hipMemcpyHostToDevice));
    LAUNCH_OK(nr_launch_fold_linear_pair(dw2, dw1, db2, db1, C, J, (bf16*)dwc, (float*)dbc, nullptr));
    HIP_OK(hipDeviceSynchronize());
    (void)hipFree(dw2); (void)hipFree(dw1); (void)hipFree(db2); (void)hipFree(db1);
    r.b = (const float*)adopt(nb, dbc, bcb);
  });
  return r;
}
// GEGLU projection [2*inner][K]: rows permuted so each 32-row group is 16 value rows then their 16 gate rows
const bf16* WeightStore::w_geglu(const std::string& key, int inner, int K) {
  return (const bf16*)convert<uint16_t>(TAG_GEGLU, key, {2 * inner, K}, (size_t)2 * inner * K, [&](const float* s, uint16_t* h) {
    for (int n = 0; n < 2 * inner; ++n) {
      const int src = geglu_src_row(n, inner);
      for (int k = 0; k < K; ++k) h[(size_t)n * K + k] = f2bf_host(s[(size_t)src * K + k]);
    }
  });
}
const float* WeightStore::b_geglu(const std::string& key, int inner) {
  return convert<float>("geglub:", key, {2 * inner}, (size_t)2 * inner, [&](const float* s, float* h) {
    for (int n = 0; n < 2 * inner; ++n) h[n] = s[geglu_src_row(n, inner)];
  });
}
// 3x3 conv weight [Cout][Cin][3][3] -> bf16 [Cout][ky][kx][Cin], or, tap_inner, in the K order of the igemm's NrGemmParams::tap_inner:
// [Cout][Cin/64][ky][kx][64]
const bf16* WeightStore::w_conv3(const std::string& key, int Cout, int Cin, bool tap_inner) {
  if (tap_inner && Cin % 64 != 0) throw NrError(NR_ERR_UNSUPPORTED, "tap-inner conv layout needs Cin % 64 == 0: " + key);
  return (const bf16*)convert<uint16_t>(tap_inner ? "conv3t:" : "conv3:", key, {Cout, Cin, 3, 3}, (size_t)Cout * 9 * Cin, [&](const float* s, uint16_t* h) {
    for (int o = 0; o < Cout; ++o)
      for (int c = 0; c < Cin; ++c)
        for (int k = 0; k < 9; ++k) {
          const size_t dst = tap_inner ? (size_t)(c / 64) * 9 * 64 + (size_t)k * 64 + (c % 64) : (size_t)k * Cin + c;
          h[(size_t)o * 9 * Cin + dst] = f2bf_host(s[((size_t)o * Cin + c) * 9 + k]);
        }
  });
}
// 3x3 conv weight [Cout][Cin][3][3] of a nearest-2x upsample conv -> its phase form [4][Cout][4][Cin] bf16 (nr_ups_phase_pack, engine.h)
const bf16* WeightStore::w_conv3_ups_phase(const std::string& key, int Cout, int Cin) {
  return (const bf16*)convert<uint16_t>("conv3up:", key, {Cout, Cin, 3, 3}, (size_t)16 * Cout * Cin, [&](const float* s, uint16_t* h) {
    nr_ups_phase_pack(s, (size_t)Cin * 9, 9, 1, Cout, Cin, h);
  });
}
// small-Cin conv weight [Cout][Cin][3][3] -> fp32 [Cin*9][Cout]
const float* WeightStore::w_conv_in(const std::string& key, int Cout, int Cin) {
  return convert<float>("convin:", key, {Cout, Cin, 3, 3}, (size_t)Cin * 9 * Cout, [&](const float* s, float* h) {
    for (int o = 0; o < Cout; ++o)
      for (int k = 0; k < Cin * 9; ++k) h[(size_t)k * Cout + o] = s[(size_t)o * Cin * 9 + k];
  });
}
// 3x3 conv weight [Cout][Cin][3][3] -> the fragment-major bf16 layout of condembed_conv: [Cout/16][KS][64 lanes][8], KS = ceil(9 Cin / 32);
// lane (fr, g) of block (T, ks) holds W[16 T + fr][k], k = 32 ks + 8 g .. + 7 = tap * Cin + c (zero beyond K = 9 Cin)
const bf16* WeightStore::w_condembed(const std::string& key, int Cout, int Cin) {
  return (const bf16*)convert<uint16_t>("cefm:", key, {Cout, Cin, 3, 3}, (size_t)nr_condembed_wfm_elems(Cin, Cout), [&](const float* s, uint16_t* h) {
    const int K = 9 * Cin, KS = (K + 31) / 32;
    for (int T = 0; T < Cout / 16; ++T)
      for (int ks = 0; ks < KS; ++ks)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int o = 16 * T + (lane & 15), k = 32 * ks + 8 * (lane >> 4) + j;
            if (k >= K) continue;
            const int tap = k / Cin, c = k % Cin;
            h[(((size_t)T * KS + ks) * 64 + lane) * 8 + j] = f2bf_host(s[((size_t)o * Cin + c) * 9 + tap]);
          }
  });
}
// elementwise sum of two fp32 vectors (the embedding's conv_out bias with conv_in.bias folded in)
const float* WeightStore::w_f32_sum(const std::string& a, const std::string& b, int64_t n) {
  check_shape(a, need(a), {n});
  check_shape(b, need(b), {n});
  const std::string name = "f32sum:" + a + "|" + b;
  return (const float*)cached(name, [&]() {
    const HostTensor& ta = data_of(a);
    const HostTensor& tb = data_of(b);
    std::vector<float> h((size_t)n);
    for (int64_t i = 0; i < n; ++i) h[i] = ta.data[i] + tb.data[i];
    return upload(name, h.data(), h.size() * 4);
  });
}
const float* WeightStore::w_f32(const std::string& key, std::initializer_list<int64_t> shape) {
  check_shape(key, need(key), shape);
  return (const float*)cached("f32:" + key, [&]() { const HostTensor& t = data_of(key); return upload("f32:" + key, t.data.data(), t.data.size() * 4); });
}
// sinusoidal temporal PE table [max_len][C]  (motion_module.py:225-239), regenerated (non-persistent buffer)
const float* WeightStore::pe_table(int C, int max_len) {
  const std::string name = "pe:" + std::to_string(C) + ":" + std::to_string(max_len);
  return (const float*)cached(name, [&]() {
    const std::vector<float> h = sinusoid_table(max_len, C);
    return upload(name, h.data(), h.size() * 4);
  });
}
// gb[f][c] = LayerNorm bias + sinusoidal positional encoding of frame f (motion_module.py:225-243), for the fused temporal-attention kernel
const float* WeightStore::b_ln_pe(const std::string& ln, int F, int C) {
  check_shape(ln + ".bias", need(ln + ".bias"), {C});
  const std::string name = "tagb:" + std::to_string(F) + ":" + ln;
  return (const float*)cached(name, [&]() {
    const HostTensor& be = data_of(ln + ".bias");
    std::vector<float> h = sinusoid_table(F, C);
    for (int pos = 0; pos < F; ++pos)
      for (int i = 0; i < C; ++i) h[(size_t)pos * C + i] = be.data[i] + h[(size_t)pos * C + i];
    return upload(name, h.data(), h.size() * 4);
  });
}

// ------------------------------------------------------------------ the weights of the fused transformer kernels
// c / b' of a LayerNorm fold (no biases) and bc of a FeedForward fold for a kernel whose stream holds the matrix: the vectors stay resident when
// the matrix goes, so they alone answer; the converter (which also checks the shapes, all the sizing pass wants) only where they are missing
WeightStore::LnW WeightStore::ln_vectors(const std::vector<std::string>& wkeys, const std::string& ln, int Neach, int K) {
  auto ic = dev.find(ln_name('c', wkeys, {}, ln)), ib = dev.find(ln_name('b', wkeys, {}, ln));
  if (!dry && ic != dev.end() && ib != dev.end()) return LnW{nullptr, (const float*)ic->second.ptr, (const float*)ib->second.ptr};
  return w_ln_linear(wkeys, {}, ln, Neach, K, false);
}
const float* WeightStore::fold_bias(const std::string& ff2, const std::string& po, int C) {
  auto ib = dev.find(fold_name('b', ff2, po));
  return (!dry && ib != dev.end()) ? (const float*)ib->second.ptr : w_fold_ff_proj(ff2, po, C).b;
}
// ffpanel.hip: one stage stream from the GEGLU matrix and the folded net.2 | proj_out matrix
WeightStore::FfFusedW WeightStore::ff_fused_weights(const std::string& ln, const std::string& ff, const std::string& po, int C) {
  const int inner = 4 * C;
  const std::string w1 = ff + ".net.0.proj.weight", ff2 = ff + ".net.2";
  check_shape(w1, need(w1), {2 * inner, C});
  FfFusedW r{};
  r.b1 = b_geglu(ff + ".net.0.proj.bias", inner); r.gamma = w_f32(ln + ".weight", C); r.beta = w_f32(ln + ".bias", C);
  bool packed_now = false;
  r.stream = (const bf16*)packed("ffs:" + w1 + "|" + ff2 + ".weight|" + ff2 + ".bias|" + po + ".weight|" + po + ".bias", nr_ff_stream_bytes(C), [&](void* d) {
    const bf16* wg = w_geglu(w1, inner, C);
    LAUNCH_OK(nr_launch_ff_stream_pack(wg, w_fold_ff_proj(ff2, po, C).w, (bf16*)d, nullptr));
    packed_now = true;
  }, {TAG_GEGLU + w1});
  if (packed_now) erase(fold_name('w', ff2, po));      // the folded matrix goes again in any case (also one an earlier plan had made), the folded bias stays
  r.bc = fold_bias(ff2, po, C);
  return r;
}
// xattn.hip: to_q and to_out as one stream
WeightStore::XattnFusedW WeightStore::xattn_fused_weights(const std::string& b, int C) {
  const std::string wq = b + ".attn2.to_q.weight", wo = b + ".attn2.to_out.0.weight";
  for (auto& k : {wq, wo}) check_shape(k, need(k), {C, C});
  const void* ws = packed("xas:" + wq + "|" + wo, nr_xattn_wstream_bytes(), [&](void* d) {
    const bf16* q = w_linear(wq, C, C);
    LAUNCH_OK(nr_launch_xattn_w_pack(q, w_linear(wo, C, C), (bf16*)d, nullptr));
  }, {TAG_LIN + wq, TAG_LIN + wo});
  return {.wstream = (const bf16*)ws, .gamma = w_f32(b + ".norm2.weight", C), .beta = w_f32(b + ".norm2.bias", C), .bo = w_f32(b + ".attn2.to_out.0.bias", C)};
}
// tattn.hip: to_q, to_k, to_v and to_out as one stream; gb = LayerNorm bias + positional encoding of the F frames
WeightStore::TattnFusedW WeightStore::tattn_fused_weights(const std::string& ln, const std::string& ab, int F, int C) {
  std::vector<std::string> wk, in;
  for (const char* wn : {".to_q.weight", ".to_k.weight", ".to_v.weight", ".to_out.0.weight"}) { wk.push_back(ab + wn); in.push_back(TAG_LIN + wk.back()); }
  for (auto& k : wk) check_shape(k, need(k), {C, C});
  const void* ws = packed("tas:" + wk[0] + "|" + wk[1] + "|" + wk[2] + "|" + wk[3], nr_tattn_stream_bytes(), [&](void* d) {
    const bf16* wm[4];
    for (int i = 0; i < 4; ++i) wm[i] = w_linear(wk[i], C, C);
    LAUNCH_OK(nr_launch_tattn_stream_pack(wm[0], wm[1], wm[2], wm[3], (bf16*)d, nullptr));
  }, in);
  return {.stream = (const bf16*)ws, .gb = b_ln_pe(ln, F, C), .gamma = w_f32(ln + ".weight", C), .bo = w_f32(ab + ".to_out.0.bias", C)};
}
// xattnw.hip: the stream from the LayerNorm-folded to_q matrix, the table from the fold's vectors
WeightStore::HeadW WeightStore::xattn_head_weights(const std::string& ln, const std::string& wq, int C) {
  if (dry) (void)ln_vectors({wq}, ln, C, C);      // shape checks in the sizing pass too
  const void* ws = packed("xaws:" + ln + "|" + wq, nr_xattnw_wstream_bytes(C), [&](void* d) {
    LAUNCH_OK(nr_launch_xattnw_w_pack(w_ln_linear({wq}, {}, ln, C, C, false).w, C, (bf16*)d, nullptr));
  }, {ln_name('w', {wq}, {}, ln)});
  const void* tb = packed("xawt:" + ln + "|" + wq, nr_xattnw_table_bytes(C), [&](void* d) {
    const LnW lw = ln_vectors({wq}, ln, C, C);
    LAUNCH_OK(nr_launch_xattnw_table_pack(lw.c, lw.b, C, (float*)d, nullptr));
  });
  return {(const bf16*)ws, (const float*)tb};
}
// tattnw.hip: the stream from the LayerNorm-folded q|k|v matrix; the head-major epilogue table (the fold's vectors + the positional-encoding projections of
// the first F positions) the kernel stages through LDS: one per frame count a handle was planned with
WeightStore::HeadW WeightStore::tattn_head_weights(const std::string& ln, const std::vector<std::string>& wqkv, int C, int F, int max_len) {
  const float* rv = pe_projection(wqkv, C, C, max_len);
  const std::string keys = ln + "|" + wqkv[0] + "|" + wqkv[1] + "|" + wqkv[2];
  const void* ws = packed("taws:" + keys, nr_tattnw_stream_bytes(C), [&](void* d) {
    LAUNCH_OK(nr_launch_tattnw_stream_pack(w_ln_linear(wqkv, {}, ln, C, C, false).w, C, (bf16*)d, nullptr));
  }, {ln_name('w', wqkv, {}, ln)});
  const void* tb = packed("tawe:" + std::to_string(max_len) + ":" + std::to_string(F) + ":" + keys, nr_tattnw_table_bytes(C, F), [&](void* d) {
    const LnW lw = ln_vectors(wqkv, ln, C, C);
    LAUNCH_OK(nr_launch_tattnw_table_pack(lw.c, lw.b, rv, C, F, (float*)d, nullptr));
  });
  return {(const bf16*)ws, (const float*)tb};
}

}  // namespace nre
