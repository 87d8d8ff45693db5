// Small / boundary kernels of the denoiser path (none of them GEMM-shaped enough for MFMA):
//   conv_in_small   : 3x3 conv from the fp32 NCFHW latent boundary (Cin = 4, or 4+1 for the SparseCtrl
//                     condition+mask) to channels-last bf16            (unet.py:405; sparse_controlnet.py:513-521)
//   conv_out_small  : 3x3 conv from channels-last bf16 (already GN+SiLU'd) to fp32 NCFHW eps (unet.py:468-470)
//   timestep_sincos : diffusers Timesteps(320, flip_sin_to_cos=True, freq_shift=0)  (unet.py:101,386; in-repo
//                     twin: generative_models/sgm/modules/diffusionmodules/util.py:207-231)
//   linear_small    : y = W act(x) + b for the handful-of-rows time-embedding MLPs (unet.py:392; resnet.py:191)
//   add_bf16        : out = a + b (ControlNet residual adds, unet.py:425-428,436-439)
//   condembed_*     : the SparseCtrl image-condition embedding (end of this file): a first conv from the fp32 condition planes, the
//                     small-channel 3x3 convs on MFMA (implicit GEMM, K = 9 Cin <= 864) and the batch / frame broadcast
#include "launchers.h"

namespace {

// ---------------------------------------------------------------------------------------------
// conv_in_small: out[n][y][x][co] = bias[co] + sum_{ci,ky,kx} wT[(ci*9+ky*3+kx)][co] * in(ci, y+ky-1, x+kx-1)
// sources: s0 fp32 [B][c0][F][H][W], s1 fp32 [B][c1][F][H][W] (may be null).  Source batch index = b % src_batch
// (CFG halves share one latent; SparseCtrl condition has batch B while the net runs 2B).
// grid (H, nimg), block 256; LDS patch [Cin][3][W+2]
// ---------------------------------------------------------------------------------------------
template <int CIN>
__global__ __launch_bounds__(256) void conv_in_small_kernel(const float* __restrict__ s0, const float* __restrict__ s1,
                                                            int c0, int c1, int src_batch, int F, int H, int W,
                                                            const float* __restrict__ wT, const float* __restrict__ bias,
                                                            const float* __restrict__ addend, int Cout,
                                                            bf16* __restrict__ out, float in_scale, float in_shift) {
  // thread = one output channel (coalesced weight reads and output stores) with its 9*CIN weights in registers,
  // register-blocked over 8 pixels of the row; the 3-row input patch sits in LDS (wave-uniform broadcast reads).
  extern __shared__ float patch[];
  constexpr int K = CIN * 9;
  const int y = blockIdx.x, n = blockIdx.y;
  const int b = (n / F) % src_batch, f = n % F;
  const int PW = W + 2;
  for (int i = threadIdx.x; i < CIN * 3 * PW; i += 256) {
    const int ci = i / (3 * PW);
    const int r = i - ci * 3 * PW;
    const int ky = r / PW, px = r - ky * PW;
    const int iy = y + ky - 1, ix = px - 1;
    float v = 0.f;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
      const float* s; int cc, cs;
      if (ci < c0) { s = s0; cc = ci; cs = c0; } else { s = s1; cc = ci - c0; cs = c1; }
      v = s[((((size_t)b * cs + cc) * F + f) * H + iy) * W + ix] * in_scale + in_shift;   // padding stays 0
    }
    patch[i] = v;
  }
  __syncthreads();
  for (int co = threadIdx.x; co < Cout; co += 256) {
    float w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = wT[(size_t)k * Cout + co];
    const float b0 = bias[co] + (addend ? addend[co] : 0.f);
    for (int x0 = 0; x0 < W; x0 += 8) {
      float acc[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = b0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int ci = k / 9, t = k - ci * 9;
        const int ky = t / 3, kx = t - ky * 3;
        const float* pr = patch + (ci * 3 + ky) * PW + x0 + kx;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += w[k] * pr[e];   // pr[e] beyond W+1 only when x0+e >= W (masked at the store)
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (x0 + e < W) out[(((size_t)n * H + y) * W + x0 + e) * Cout + co] = (bf16)acc[e];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// conv_out_small: one wave per output pixel, Cout <= 4.  w: [Cout][9][Cin] bf16.  out fp32 [B][Cout][F][H][W]
// ---------------------------------------------------------------------------------------------
template <int COUT>
__global__ __launch_bounds__(256) void conv_out_small_kernel(const bf16* __restrict__ x, int Cin, int nimg, int F, int H,
                                                             int W, const bf16* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             float out_mul, float out_add, int clamp01) {
  const int lane = threadIdx.x & 63;
  const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long npix = (long long)nimg * H * W;
  if (pix >= npix) return;
  const int n = (int)(pix / (H * W));
  const int r = (int)(pix - (long long)n * H * W);
  const int y = r / W, xx = r - y * W;
  const int CP = Cin >> 3;
  float acc[COUT];
#pragma unroll
  for (int o = 0; o < COUT; ++o) acc[o] = 0.f;
  for (int id = lane; id < 9 * CP; id += 64) {
    const int tap = id / CP, cc = (id - tap * CP) << 3;
    const int ky = tap / 3, kx = tap - ky * 3;
    const int iy = y + ky - 1, ix = xx + kx - 1;
    if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
    const bf16x8 v = *(const bf16x8*)(x + (((size_t)n * H + iy) * W + ix) * Cin + cc);
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
      const bf16x8 ww = *(const bf16x8*)(w + ((size_t)o * 9 + tap) * Cin + cc);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[o] += (float)v[e] * (float)ww[e];
    }
  }
#pragma unroll
  for (int o = 0; o < COUT; ++o) acc[o] = wave_sum(acc[o]);
  if (lane == 0) {
    const int b = n / F, f = n - b * F;
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
      // image post-scaling of the callers: (x / 2 + 0.5).clamp(0, 1) pipeline_animation.py:252; clamp(x*.8+.2) utils.py:348
      float v = (acc[o] + bias[o]) * out_mul + out_add;
      if (clamp01) v = fminf(fmaxf(v, 0.f), 1.f);
      out[((((size_t)b * COUT + o) * F + f) * H + y) * W + xx] = v;
    }
  }
}

// post_quant_conv (1x1, C <= 8) on the fp32 NCHW latent: out[n][co][p] = qb[co] + sum_ci Q[co][ci] * (z[n][ci][p] * scale)
// (sgm/models/autoencoder.py:459,492; the 1/scale_factor of diffusion.py:119 / pipeline_animation.py:245 is `scale`)
__global__ void post_quant_kernel(const float* __restrict__ z, float scale, const float* __restrict__ Q,
                                  const float* __restrict__ qb, float* __restrict__ out, int nimg, int C, int hw) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)nimg * hw) return;
  const int n = (int)(idx / hw), p = (int)(idx - (long long)n * hw);
  float v[8];
  for (int c = 0; c < C; ++c) v[c] = z[((size_t)n * C + c) * hw + p] * scale;
  for (int co = 0; co < C; ++co) {
    float a = qb[co];
    for (int c = 0; c < C; ++c) a += Q[co * C + c] * v[c];
    out[((size_t)n * C + co) * hw + p] = a;
  }
}

// DiagonalGaussianDistribution.sample / .mode (sgm/modules/distributions/distributions.py:24-42; diffusers twin used
// by scripts/neuroclips_video.py:267): moments [n][2z][hw] -> out[n][z][hw] = (mean + exp(0.5*clamp(logvar,-30,20)) * noise) * scale
__global__ void gaussian_sample_kernel(const float* __restrict__ moments, const float* __restrict__ noise, float* __restrict__ out,
                                       long long total, int zc, int hw, float scale) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long long n = idx / ((long long)zc * hw);
  const long long r = idx - n * (long long)zc * hw;
  const float mean = moments[n * 2 * zc * hw + r];
  float v = mean;
  if (noise) {
    const float lv = fminf(fmaxf(moments[n * 2 * zc * hw + (long long)zc * hw + r], -30.f), 20.f);
    v += expf(0.5f * lv) * noise[idx];
  }
  out[idx] = v * scale;
}

// row softmax of fp32 scores -> bf16 probabilities: P[r][:] = softmax(S[r][:] * scale).  One 256-thread block per row.
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ S, bf16* __restrict__ P, int L, float scale_log2e) {
  __shared__ float red[4];
  const float* s = S + (size_t)blockIdx.x * L;
  bf16* o = P + (size_t)blockIdx.x * L;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float m = -INFINITY;
  for (int i = threadIdx.x * 4; i < L; i += 1024) {
    const f32x4 v = *(const f32x4*)(s + i);
    m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
  }
  m = wave_max(m);
  if (lane == 0) red[wv] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * scale_log2e;
  __syncthreads();
  float l = 0.f;
  for (int i = threadIdx.x * 4; i < L; i += 1024) {
    const f32x4 v = *(const f32x4*)(s + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) l += exp2f(v[e] * scale_log2e - m);
  }
  l = wave_sum(l);
  if (lane == 0) red[wv] = l;
  __syncthreads();
  const float inv = 1.f / (red[0] + red[1] + red[2] + red[3]);
  for (int i = threadIdx.x * 4; i < L; i += 1024) {
    const f32x4 v = *(const f32x4*)(s + i);
    bf16x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (bf16)(exp2f(v[e] * scale_log2e - m) * inv);
    *(bf16x4*)(o + i) = r;
  }
}

// t: [M] fp32 timesteps -> out [M][dim] = [cos(t*f_i) | sin(t*f_i)], f_i = exp(-ln(1e4) * i / half), half = dim/2
__global__ void timestep_sincos_kernel(const float* __restrict__ t, int M, int dim, float* __restrict__ out) {
  const int half = dim >> 1;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M * half) return;
  const int m = idx / half, i = idx - m * half;
  const float freq = expf(-9.210340371976184f * (float)i / (float)half);
  const float a = t[m] * freq;
  out[(size_t)m * dim + i] = cosf(a);
  out[(size_t)m * dim + half + i] = sinf(a);
}

// y[m][n] = sum_k act(x[m][k]) * W[n][k] + b[n];  one wave per (n, 16-row slab of m), K % 8 == 0.  act: 0 none, 1 SiLU (on input)
// out_act: 0 none, 1 SiLU (on output)
__global__ __launch_bounds__(256) void linear_small_kernel(const float* __restrict__ x, int M, int K,
                                                           const bf16* __restrict__ W, const float* __restrict__ b, int N,
                                                           int in_act, int out_act, float* __restrict__ y,
                                                           const float* __restrict__ addend) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  {   // blockIdx.y: 16-row slab of the batch
    const int m0 = blockIdx.y * 16;
    x += (size_t)m0 * K; y += (size_t)m0 * N;
    if (addend) addend += (size_t)m0 * N;
    M = M - m0 < 16 ? M - m0 : 16;
  }
  float acc[16];
#pragma unroll
  for (int m = 0; m < 16; ++m) acc[m] = 0.f;
  for (int k0 = lane * 8; k0 < K; k0 += 64 * 8) {
    const bf16x8 w = *(const bf16x8*)(W + (size_t)n * K + k0);
    float wf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) wf[e] = (float)w[e];
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      if (m < M) {
        const f32x4 x0 = *(const f32x4*)(x + (size_t)m * K + k0), x1 = *(const f32x4*)(x + (size_t)m * K + k0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float a = x0[e], b2 = x1[e];
          if (in_act) { a = silu_f(a); b2 = silu_f(b2); }
          acc[m] += a * wf[e] + b2 * wf[4 + e];
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    if (m < M) {
      float v = wave_sum(acc[m]);
      if (lane == 0) {
        v += b ? b[n] : 0.f;
        if (addend) v += addend[(size_t)m * N + n];
        if (out_act) v = silu_f(v);
        y[(size_t)m * N + n] = v;
      }
    }
  }
}

__global__ void add_bf16_kernel(const bf16* __restrict__ a, const bf16* __restrict__ b, bf16* __restrict__ out,
                                long long n8) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const bf16x8 va = ((const bf16x8*)a)[i], vb = ((const bf16x8*)b)[i];
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (bf16)((float)va[e] + (float)vb[e]);
  nr_store16((bf16*)out + 8 * i, o);
}

__global__ __launch_bounds__(256) void add_bf16_multi_kernel(NrAddMulti p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n8_end[p.count - 1]) return;
  int t = 0;
#pragma unroll
  for (int k = 0; k < 15; ++k) t += (k < p.count - 1 && i >= p.n8_end[k]) ? 1 : 0;
  const long long j = i - (t ? p.n8_end[t - 1] : 0);
  const bf16x8 va = ((const bf16x8*)p.dst[t])[j], vb = ((const bf16x8*)p.src[t])[j];
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (bf16)((float)va[e] + (float)vb[e]);
  nr_store16(p.dst[t] + 8 * j, o);
}

// fp32 [rows][C] -> bf16 [rows][C]
__global__ void f32_to_bf16_kernel(const float* __restrict__ a, bf16* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (bf16)a[i];
}

// CLIPTextEmbeddings (transformers CLIPTextModel, called by pipeline_neuroclips.py:153-240 _encode_prompt):
// out[m][:] = token_embedding[ids[m]][:] + position_embedding[m % L][:]   (fp32 tables, one rounding to bf16)
__global__ void clip_embed_kernel(const int* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                  bf16* __restrict__ out, int M, int L, int C, int vocab) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4 = C >> 2;
  if (idx >= (long long)M * c4) return;
  const int m = (int)(idx / c4), c = (int)(idx - (long long)m * c4) << 2;
  int id = ids[m];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const f32x4 a = *(const f32x4*)(tok + (size_t)id * C + c);
  const f32x4 b = *(const f32x4*)(pos + (size_t)(m % L) * C + c);
  bf16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (bf16)(a[e] + b[e]);
  *(bf16x4*)(out + (size_t)m * C + c) = o;
}

__global__ void bf16_to_f32_kernel(const bf16* __restrict__ a, float* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (float)a[i];
}

// Weight-conversion time only (not on the denoising path): two consecutive Linears with nothing but a residual add between them,
//   out = x + b2 + W2 (t + b1 + W1 g)   (FeedForward.net.2 then proj_out; motion_module_new.py:441-471, attention.py:137-141)
// are folded into ONE GEMM over the concatenated operand [t | g]:  Wc = [W2 | W2 W1] (bf16), bc = b2 + W2 b1 (fp32).
// w2: [C][C], w1: [C][J] (both fp32, row-major); wc: [C][C + J].  grid (ceil((C + J) / 256), C).
__global__ __launch_bounds__(256) void fold_linear_pair_kernel(const float* __restrict__ w2, const float* __restrict__ w1,
                                                               const float* __restrict__ b2, const float* __restrict__ b1, int C, int J,
                                                               bf16* __restrict__ wc, float* __restrict__ bc) {
  const int n = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  const float* w2r = w2 + (size_t)n * C;
  if (col < C) {
    wc[(size_t)n * (C + J) + col] = (bf16)w2r[col];
  } else if (col < C + J) {
    const int j = col - C;
    float a = 0.f;
    for (int c = 0; c < C; ++c) a = fmaf(w2r[c], w1[(size_t)c * J + j], a);
    wc[(size_t)n * (C + J) + col] = (bf16)a;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float a = b2[n];
    for (int c = 0; c < C; ++c) a = fmaf(w2r[c], b1[c], a);
    bc[n] = a;
  }
}

}  // namespace

// test-hook layout converts of the leaf-module handles (engine.hip build_leaf): fp32 "b c f h w" <-> bf16 channels-last frame-images
// [b*F + f][hw][C].  One thread per (image, pixel, channel); sized for fixtures, not for speed.
static __global__ void ncfhw_to_nhwc_kernel(const float* __restrict__ src, bf16* __restrict__ dst, int C, int F, int HW, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const long long pix = i / C;
  const int p = (int)(pix % HW);
  const long long n = pix / HW;
  const int f = (int)(n % F);
  const long long b = n / F;
  dst[i] = (bf16)src[((b * C + c) * F + f) * HW + p];
}
static __global__ void nhwc_to_ncfhw_kernel(const bf16* __restrict__ src, float* __restrict__ dst, int C, int F, int HW, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int p = (int)(i % HW);
  long long r = i / HW;
  const int f = (int)(r % F);
  r /= F;
  const int c = (int)(r % C);
  const long long b = r / C;
  dst[i] = (float)src[((b * F + f) * HW + p) * C + c];
}

// dst[b][fd][:] = src[b][map[fd]][:]  (frame-images of frame_elems bf16, 16-byte pieces): the reduce / expand steps of SparseCtrl's
// identical-frame evaluation (engine.hip build(): frames without a condition are identical until the first motion module)
struct NrFrameMap { int v[64]; };
static __global__ __launch_bounds__(256) void frame_gather_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int Fs, int Fd, long long f16,
                                                                   NrFrameMap map, long long total16) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total16) return;
  const long long img = i / f16, r = i - img * f16;
  const long long b = img / Fd;
  const int fd = (int)(img - b * Fd);
  dst[i] = src[(b * Fs + map.v[fd]) * f16 + r];
}
extern "C" int nr_launch_frame_gather(const bf16* src, bf16* dst, int B, int Fs, int Fd, long long frame_elems, const int* map, hipStream_t stream) {
  if (Fd > 64 || frame_elems % 8 != 0) return 1;
  NrFrameMap m;
  for (int i = 0; i < 64; ++i) m.v[i] = i < Fd ? map[i] : 0;
  const long long f16 = frame_elems / 8, total16 = (long long)B * Fd * f16;
  hipLaunchKernelGGL(frame_gather_kernel, dim3((unsigned)((total16 + 255) / 256)), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst, Fs, Fd, f16, m, total16);
  return 0;
}

extern "C" int nr_launch_ncfhw_to_nhwc(const float* src, bf16* dst, int B, int C, int F, int HW, hipStream_t stream) {
  const long long total = (long long)B * C * F * HW;
  hipLaunchKernelGGL(ncfhw_to_nhwc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, dst, C, F, HW, total);
  return 0;
}
extern "C" int nr_launch_nhwc_to_ncfhw(const bf16* src, float* dst, int B, int C, int F, int HW, hipStream_t stream) {
  const long long total = (long long)B * C * F * HW;
  hipLaunchKernelGGL(nhwc_to_ncfhw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, dst, C, F, HW, total);
  return 0;
}

extern "C" int nr_launch_fold_linear_pair(const float* w2, const float* w1, const float* b2, const float* b1, int C, int J, bf16* wc,
                                          float* bc, hipStream_t stream) {
  hipLaunchKernelGGL(fold_linear_pair_kernel, dim3((unsigned)((C + J + 255) / 256), (unsigned)C), dim3(256), 0, stream, w2, w1, b2, b1, C, J,
                     wc, bc);
  return 0;
}

extern "C" int nr_launch_clip_embed(const int* ids, const float* tok, const float* pos, bf16* out, int M, int L, int C, int vocab,
                                    hipStream_t stream) {
  if (C % 4 != 0) return 1;
  const long long total = (long long)M * (C / 4);
  hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ids, tok, pos, out, M, L, C, vocab);
  return 0;
}

extern "C" int nr_launch_bf16_to_f32(const bf16* a, float* out, long long n, hipStream_t stream) {
  hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a, out, n);
  return 0;
}

extern "C" int nr_launch_conv_in_small(const float* s0, const float* s1, int c0, int c1, int src_batch, int nimg, int F,
                                       int H, int W, const float* wT, const float* bias, const float* addend, int Cout,
                                       bf16* out, float in_scale, float in_shift, hipStream_t stream) {
  const size_t shm = ((size_t)(c0 + c1) * 3 * (W + 2) + 16) * sizeof(float);   // +16: masked over-read of the last row
  if (shm > 60000) return 1;
  if (c0 + c1 == 4)
    hipLaunchKernelGGL((conv_in_small_kernel<4>), dim3(H, nimg), dim3(256), shm, stream, s0, s1, c0, c1, src_batch, F, H, W, wT,
                       bias, addend, Cout, out, in_scale, in_shift);
  else if (c0 + c1 == 5)
    hipLaunchKernelGGL((conv_in_small_kernel<5>), dim3(H, nimg), dim3(256), shm, stream, s0, s1, c0, c1, src_batch, F, H, W, wT,
                       bias, addend, Cout, out, in_scale, in_shift);
  else if (c0 + c1 == 3)
    hipLaunchKernelGGL((conv_in_small_kernel<3>), dim3(H, nimg), dim3(256), shm, stream, s0, s1, c0, c1, src_batch, F, H, W, wT,
                       bias, addend, Cout, out, in_scale, in_shift);
  else
    return 2;
  return 0;
}

extern "C" int nr_launch_conv_out_small(const bf16* x, int Cin, int nimg, int F, int H, int W, const bf16* w,
                                        const float* bias, int Cout, float* out, float out_mul, float out_add, int clamp01, hipStream_t stream) {
  if (Cin % 8 != 0) return 1;
  const long long npix = (long long)nimg * H * W;
  const unsigned blocks = (unsigned)((npix + 3) / 4);
  if (Cout == 4)
    hipLaunchKernelGGL((conv_out_small_kernel<4>), dim3(blocks), dim3(256), 0, stream, x, Cin, nimg, F, H, W, w, bias, out, out_mul, out_add, clamp01);
  else if (Cout == 8)
    hipLaunchKernelGGL((conv_out_small_kernel<8>), dim3(blocks), dim3(256), 0, stream, x, Cin, nimg, F, H, W, w, bias, out, out_mul, out_add, clamp01);
  else if (Cout == 3)
    hipLaunchKernelGGL((conv_out_small_kernel<3>), dim3(blocks), dim3(256), 0, stream, x, Cin, nimg, F, H, W, w, bias, out, out_mul, out_add, clamp01);
  else
    return 2;
  return 0;
}

extern "C" int nr_launch_post_quant(const float* z, float scale, const float* Q, const float* qb, float* out, int nimg, int C,
                                    int hw, hipStream_t stream) {
  if (C > 8) return 1;
  const long long total = (long long)nimg * hw;
  hipLaunchKernelGGL(post_quant_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, z, scale, Q, qb, out, nimg, C, hw);
  return 0;
}

extern "C" int nr_launch_gaussian_sample(const float* moments, const float* noise, float* out, int n, int zc, int hw, float scale,
                                         hipStream_t stream) {
  const long long total = (long long)n * zc * hw;
  hipLaunchKernelGGL(gaussian_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, moments, noise, out,
                     total, zc, hw, scale);
  return 0;
}

extern "C" int nr_launch_softmax_rows(const float* S, bf16* P, int rows, int L, float scale, hipStream_t stream) {
  if (L % 4 != 0) return 1;
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(rows), dim3(256), 0, stream, S, P, L, scale * 1.4426950408889634f);
  return 0;
}

extern "C" int nr_launch_timestep_sincos(const float* t, int M, int dim, float* out, hipStream_t stream) {
  const int total = M * (dim / 2);
  hipLaunchKernelGGL(timestep_sincos_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, t, M, dim, out);
  return 0;
}

extern "C" int nr_launch_linear_small(const float* x, int M, int K, const bf16* W, const float* b, int N, int in_act,
                                      int out_act, float* y, const float* addend, hipStream_t stream) {
  if (M <= 0 || K % 8 != 0) return 1;
  hipLaunchKernelGGL(linear_small_kernel, dim3((N + 3) / 4, (M + 15) / 16), dim3(256), 0, stream, x, M, K, W, b, N, in_act, out_act, y,
                     addend);
  return 0;
}

extern "C" int nr_launch_add_bf16(const bf16* a, const bf16* b, bf16* out, long long n, hipStream_t stream) {
  if (n % 8 != 0) return 1;
  const long long n8 = n / 8;
  hipLaunchKernelGGL(add_bf16_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, stream, a, b, out, n8);
  return 0;
}

extern "C" int nr_launch_add_bf16_multi(const NrAddMulti* p, hipStream_t stream) {
  if (p->count <= 0 || p->count > 16) return 1;
  const long long total = p->n8_end[p->count - 1];
  hipLaunchKernelGGL(add_bf16_multi_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, *p);
  return 0;
}

extern "C" int nr_launch_f32_to_bf16(const float* a, bf16* out, long long n, hipStream_t stream) {
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a, out, n);
  return 0;
}

// =============================================================================================
// SparseCtrl image-condition embedding (condembed_*) (SparseControlNetConditioningEmbedding, animatediff/models/sparse_controlnet.py:49-82):
// eight 3x3 pad-1 convolutions from the RGB condition + mask at 8x the latent resolution down to the latent grid, SiLU after every
// conv but the last.  Three kernels:
//   condembed_in    : the first conv (Cin = conditioning_channels + 1 <= 8, Cout = 16 / 32) straight from the fp32 NCFHW condition and
//                     mask planes (concatenated on the fly, as conv_in_small above), plain FMA, one thread per output pixel.
//                     The frames it runs on come from a map: with the identical-frame evaluation only the conditioned frames + one
//                     representative of the rest are embedded (the engine's n_cond_frames).
//   condembed_conv  : the small-channel convs (Cin 16 .. 256, stride 1 / 2) as an implicit GEMM on v_mfma_f32_16x16x32_bf16.  K runs
//                     (tap, channel) with the channel fastest; Cin % 8 == 0, so the 8 bf16 of a lane's B fragment are one 16-byte load
//                     of one input pixel, and a 32-deep k-step covers two taps at Cin = 16 (the K = 9 Cin tail is zero-padded).
//                     Weights are fragment-major [Cout/16][KS][64 lanes][8] (KS = ceil(9 Cin / 32)): a wave's A operand of one k-step
//                     is one contiguous KiB, read through L2 (the largest layer, 96 -> 256, is 442 KiB).  The activations are
//                     read straight from global memory into the B fragments; a tap re-reads its neighbours' pixels from L1/L2.
//                     Each wave computes 32 output pixels x 16 NT output channels.
//   condembed_bcast : x[b][f] = emb[b % cond_batch][emap[f]] (+ addend[b][f]): the per-condition-image embedding broadcast over the
//                     CFG / grouped batch and over the frames that share one embedding.
// =============================================================================================

namespace {

typedef __attribute__((ext_vector_type(8))) short i16x8;

constexpr int CE_MAX_FRAMES = 64;
struct CeFrameMap { int f[CE_MAX_FRAMES]; };

// ---------------------------------------------------------------------------------------------
// first conv: out[n][y][x][co] = silu(bias[co] + sum_{ci,ky,kx} wT[ci*9+ky*3+kx][co] * in(ci, y+ky-1, x+kx-1))
// in(ci < c0) = cond[b][ci][f][..], in(c0) = mask[b][0][f][..]; n = b * Fe + e, f = fmap[e].  grid (ceil(H*W / 256), nimg)
// ---------------------------------------------------------------------------------------------
template <int COUT>
__global__ __launch_bounds__(256) void condembed_in_kernel(const float* __restrict__ cond, const float* __restrict__ mask, int c0,
                                                           int F, int H, int W, CeFrameMap fmap, int Fe,
                                                           const float* __restrict__ wT, const float* __restrict__ bias,
                                                           bf16* __restrict__ out) {
  __shared__ float sw[8 * 9 * COUT];
  __shared__ float sb[COUT];
  const int cin = c0 + 1;
  for (int i = threadIdx.x; i < cin * 9 * COUT; i += 256) sw[i] = wT[i];
  if (threadIdx.x < COUT) sb[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const int n = blockIdx.y;
  const int b = n / Fe, f = fmap.f[n - b * Fe];
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= H * W) return;
  const int y = pix / W, x = pix - y * W;
  float acc[COUT];
#pragma unroll
  for (int o = 0; o < COUT; ++o) acc[o] = sb[o];
  for (int ci = 0; ci < cin; ++ci) {
    const float* src = ci < c0 ? cond + (((size_t)b * c0 + ci) * F + f) * H * W : mask + ((size_t)b * F + f) * H * W;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
      const float v = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? src[(size_t)iy * W + ix] : 0.f;
      const float* wr = sw + (ci * 9 + t) * COUT;
#pragma unroll
      for (int o = 0; o < COUT; ++o) acc[o] += v * wr[o];
    }
  }
  bf16* op = out + ((size_t)n * H * W + pix) * COUT;
#pragma unroll
  for (int o8 = 0; o8 < COUT; o8 += 8) {
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (bf16)silu_f(acc[o8 + e]);
    nr_store16(op + o8, v);
  }
}

// ---------------------------------------------------------------------------------------------
// small-channel 3x3 conv, pad 1, stride S: out[p][co] = act(bias[co] + sum_k W[co][k] * im2col(x)[p][k]), k = tap * CIN + c.
// Transposed MFMA as in gemm.hip (weights = A operand, pixels = B operand): lane (fr = l & 15, g = l >> 4) holds output channels
// 16 T + 4 g .. + 3 of pixel 16 j + fr, stored as one 8-byte vector.  Block = 4 waves x 32 pixels; grid (ceil(M / 128), Cout / (16 NT)).
// ---------------------------------------------------------------------------------------------
template <int CIN, int S, int NT>
__global__ __launch_bounds__(256) void condembed_conv_kernel(const bf16* __restrict__ x, int H, int W, int OH, int OW, int M,
                                                             const bf16* __restrict__ wfm, const float* __restrict__ bias, int Cout,
                                                             int silu, bf16* __restrict__ out) {
  constexpr int K = 9 * CIN;
  constexpr int KS = (K + 31) / 32;
  constexpr int MT = 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int p0 = (blockIdx.x * 4 + wave) * (16 * MT);
  const int T0 = blockIdx.y * NT;
  if (p0 >= M) return;
  // per lane: the pixel of its B-fragment column in each of the MT pixel tiles
  int pn[MT], py[MT], px[MT];
  bool pv[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    const int p = p0 + 16 * j + fr;
    pv[j] = p < M;
    const int pp = pv[j] ? p : 0;
    const int n = pp / (OH * OW), r = pp - n * OH * OW;
    const int oy = r / OW, ox = r - oy * OW;
    pn[j] = n; py[j] = oy * S - 1; px[j] = ox * S - 1;
  }
  f32x4 acc[NT][MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const i16x8* wl = (const i16x8*)wfm + (size_t)T0 * KS * 64 + lane;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int k0 = 32 * ks + 8 * g;
    const int tap = k0 / CIN, c = k0 - tap * CIN;
    const int ky = tap / 3, kx = tap - ky * 3;
    i16x8 bfr[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int iy = py[j] + ky, ix = px[j] + kx;
      const bool ok = pv[j] && k0 < K && iy >= 0 && iy < H && ix >= 0 && ix < W;
      bfr[j] = ok ? *(const i16x8*)(x + (((size_t)pn[j] * H + iy) * W + ix) * CIN + c) : i16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const i16x8 a = wl[((size_t)i * KS + ks) * 64];
#pragma unroll
      for (int j = 0; j < MT; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bfr[j]), acc[i][j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int co = (T0 + i) * 16 + 4 * g;
    const f32x4 bv = *(const f32x4*)(bias + co);
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      if (!pv[j]) continue;
      f32x4 v = acc[i][j] + bv;
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (bf16)(silu ? silu_f(v[e]) : v[e]);
      nr_store8(out + (size_t)(p0 + 16 * j + fr) * Cout + co, o);
    }
  }
}

// x[n = b * F + f] = emb[(b % cb) * Fe + emap[f]] (+ add[n]), img8 = 16-byte words per image
__global__ __launch_bounds__(256) void condembed_bcast_kernel(const bf16x8* __restrict__ emb, int cb, int Fe, CeFrameMap emap, int F,
                                                              long long img8, const bf16x8* __restrict__ add, bf16x8* __restrict__ out,
                                                              long long total8) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total8) return;
  const long long n = i / img8, r = i - n * img8;
  const int b = (int)(n / F), f = (int)(n - (long long)b * F);
  bf16x8 v = emb[((long long)(b % cb) * Fe + emap.f[f]) * img8 + r];
  if (add) {
    const bf16x8 a = add[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (bf16)((float)v[e] + (float)a[e]);
  }
  out[i] = v;
}

template <int CIN, int S>
int launch_conv(int NT, dim3 grid, hipStream_t s, const bf16* x, int H, int W, int OH, int OW, int M, const bf16* w, const float* b,
                int Cout, int silu, bf16* out) {
  if (NT == 1) hipLaunchKernelGGL((condembed_conv_kernel<CIN, S, 1>), grid, dim3(256), 0, s, x, H, W, OH, OW, M, w, b, Cout, silu, out);
  else if (NT == 2) hipLaunchKernelGGL((condembed_conv_kernel<CIN, S, 2>), grid, dim3(256), 0, s, x, H, W, OH, OW, M, w, b, Cout, silu, out);
  else return 3;
  return 0;
}

}  // namespace

extern "C" {

int nr_condembed_in_supported(int cin, int Cout) { return cin >= 1 && cin <= 8 && (Cout == 16 || Cout == 32); }

// nsrc condition images x Fe frames (frames fmap[0..Fe) of the F-frame condition) -> [nsrc * Fe][H][W][Cout] bf16
int nr_launch_condembed_in(const float* cond, const float* mask, int c0, int nsrc, int F, int H, int W, const int* fmap, int Fe,
                           const float* wT, const float* bias, int Cout, bf16* out, hipStream_t s) {
  if (!nr_condembed_in_supported(c0 + 1, Cout) || Fe < 1 || Fe > CE_MAX_FRAMES || nsrc < 1) return 1;
  CeFrameMap m;
  for (int e = 0; e < Fe; ++e) {
    if (fmap[e] < 0 || fmap[e] >= F) return 2;
    m.f[e] = fmap[e];
  }
  const dim3 grid((unsigned)((H * W + 255) / 256), (unsigned)(nsrc * Fe));
  if (Cout == 16) hipLaunchKernelGGL(condembed_in_kernel<16>, grid, dim3(256), 0, s, cond, mask, c0, F, H, W, m, Fe, wT, bias, out);
  else hipLaunchKernelGGL(condembed_in_kernel<32>, grid, dim3(256), 0, s, cond, mask, c0, F, H, W, m, Fe, wT, bias, out);
  return 0;
}

int nr_condembed_conv_supported(int Cin, int stride, int Cout) {
  const bool cin_ok = Cin == 16 || Cin == 32 || Cin == 64 || Cin == 96 || Cin == 128 || Cin == 256;
  return cin_ok && (stride == 1 || stride == 2) && Cout % 16 == 0 && Cout > 0;
}

// bf16 elements of the fragment-major weight [Cout/16][ceil(9 Cin / 32)][64][8]
long long nr_condembed_wfm_elems(int Cin, int Cout) { return (long long)Cout * ((9 * Cin + 31) / 32) * 32; }

int nr_launch_condembed_conv(const bf16* x, int nimg, int H, int W, int Cin, int stride, const bf16* wfm, const float* bias, int Cout,
                             int silu, bf16* out, hipStream_t s) {
  if (!nr_condembed_conv_supported(Cin, stride, Cout) || nimg < 1) return 1;
  const int OH = stride == 2 ? (H - 1) / 2 + 1 : H, OW = stride == 2 ? (W - 1) / 2 + 1 : W;
  const long long M = (long long)nimg * OH * OW;
  if (M >= (1ll << 31) / 256) return 2;     // pixel * Cout (Cout <= 256) stays below 2^31
  const int NT = Cout % 32 == 0 ? 2 : 1;
  const dim3 grid((unsigned)((M + 127) / 128), (unsigned)(Cout / (16 * NT)));
  const int m = (int)M;
#define CE_CASE(C)                                                                                                  \
  if (Cin == C)                                                                                                     \
    return stride == 1 ? launch_conv<C, 1>(NT, grid, s, x, H, W, OH, OW, m, wfm, bias, Cout, silu, out)            \
                       : launch_conv<C, 2>(NT, grid, s, x, H, W, OH, OW, m, wfm, bias, Cout, silu, out);
  CE_CASE(16) CE_CASE(32) CE_CASE(64) CE_CASE(96) CE_CASE(128) CE_CASE(256)
#undef CE_CASE
  return 1;
}

int nr_launch_condembed_bcast(const bf16* emb, int cb, int Fe, const int* emap, int B, int F, long long img_elems, const bf16* add,
                              bf16* out, hipStream_t s) {
  if (img_elems % 8 != 0 || cb < 1 || B % cb != 0 || F > CE_MAX_FRAMES) return 1;
  CeFrameMap m;
  for (int f = 0; f < F; ++f) {
    if (emap[f] < 0 || emap[f] >= Fe) return 2;
    m.f[f] = emap[f];
  }
  const long long img8 = img_elems / 8, total8 = (long long)B * F * img8;
  hipLaunchKernelGGL(condembed_bcast_kernel, dim3((unsigned)((total8 + 255) / 256)), dim3(256), 0, s, (const bf16x8*)emb, cb, Fe, m, F,
                     img8, (const bf16x8*)add, (bf16x8*)out, total8);
  return 0;
}

}  // extern "C"
