// Training and autograd kernels of the wide shapes (TNP_WIDE_SHAPES x levels
// 2..8: 16 x 5, 32 x 3, 32 x 4 -- K = 65 / 97): the same three kernels, the
// same arguments and the same packed gradient layout as train_net.h, whose
// one-point-per-lane form (every activation of a point in registers, one
// wave reduction per parameter) does not fit 32-wide layers.  Here one wave
// handles 64 points together and the layers run on the matrix cores
// (v_mfma_f32_16x16x4_f32, exact fp32):
//   forward / tangent layer   D = W . X^T, net_device.h mfma_layer: the
//                             activations stay in the B-operand layout
//   transposed layer          delta_{l-1} = D_{l-1} W_l^T delta_l, u = W_0^T
//                             delta_0: the same MFMA, the A operand read from
//                             the LDS weights in transposed order
//   weight gradient           dW_l[j][k] = sum_row delta_l[row][j] c_{l-1}[row][k],
//                             c_l = kappa h_l + mu h'_l (c_{-1} = kappa e + mu a;
//                             the forward VJP: c = h): a 16 x 16 tile of dW is
//                             16 chained MFMAs over the wave's 64 rows, both
//                             operands read from plane-major LDS stages
// The encoding (cell, corners, table atomics, the Hessian term) stays one
// point per lane (train_net.h tcell_of / tcorner_of).  Per wave, LDS holds
// the c planes of every layer (16 + (NL - 1) H planes of MST floats), one
// layer's delta planes (H) and a ReLU mask word per layer in registers;
// delta is recomputed layer by layer once kappa and mu are known.  Bias and
// output-layer gradients are 16-lane shuffle sums of the accumulator layout.
// Dead rows (i >= n) carry kappa = mu = 0 (c = 0) or a zero delta, so they
// add exact zeros to every product; no MFMA is branched around.
//
// Workgroup: TW_WAVES = 2 waves (128 points).  The 32 x 4 net at 8 levels
// needs 2 x 2722 floats of weights and gradients plus 2 x (112 + 32) planes
// = 114 KB of the CU's 160 KB; a third wave would not fit.  The 65-plane
// shapes (71 - 85 KB) use the same size.
// Summation order is free (train_net.h header).
#pragma once
#include "train_net.h"

namespace {

constexpr int TW_WAVES = 2;
constexpr int TW_BLOCK = 64 * TW_WAVES;

template <int LV, int H, int NL>
struct WideShape {
  static constexpr int IN = 2 * LV, NH = NL - 1, NG = H / 16;
  static constexpr int S0 = (IN + 3) / 4, SH = H / 4, SM = S0 > SH ? S0 : SH;
  static constexpr int NW = NetShape<LV, H, NL>::NW;
  static constexpr int OL = NW - 2 * H - 2;  // the output layer's offset in the packed layout
  static constexpr int DPL = H;              // delta planes (also the 16-plane row <-> lane-layout transposes)
  static constexpr int CPL = 16 + NH * H;    // c planes: c_{-1} (IN of 16), then c_0 .. c_{NH-1}
  static_assert(H % 16 == 0 && H <= 32 && IN <= 16, "mask words of 32 bits, one input tile");
};

// sum over the 16 lanes r of one q group (lane = 16 q + r)
__device__ __forceinline__ float row_sum16(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// bit of accumulator element (G, g, b) in a layer's ReLU mask word
__device__ __forceinline__ bool mask_bit(uint32_t m, int G, int g, int b) { return (m >> (16 * G + 4 * g + b)) & 1u; }

// the encoding of one point (TPass::run's first loop)
template <int LV>
__device__ __forceinline__ void tw_encode(const NetDev& net, const float x[3], float (&e)[2 * LV]) {
  const float2* tab = reinterpret_cast<const float2*>(net.table);
#pragma unroll
  for (int l = 0; l < LV; ++l) {
    float t[3];
    uint32_t g[3];
    tcell_of(net, l, x, t, g);
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const TCorner k = tcorner_of(net, l, t, g, c);
      const float2 v = tab[k.idx];
      s0 += k.w * v.x;
      s1 += k.w * v.y;
    }
    e[2 * l] = s0;
    e[2 * l + 1] = s1;
  }
}

// d/dx of (u . e) for an upstream u of the encoding, x in [-1, 1] (TPass::run's last loop)
template <int LV>
__device__ __forceinline__ void tw_encode_dx(const NetDev& net, const float x[3], const float (&u)[2 * LV],
                                             float gz[3]) {
  const float2* tab = reinterpret_cast<const float2*>(net.table);
  gz[0] = gz[1] = gz[2] = 0.f;
#pragma unroll
  for (int l = 0; l < LV; ++l) {
    float t[3];
    uint32_t g[3];
    tcell_of(net, l, x, t, g);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const TCorner k = tcorner_of(net, l, t, g, c);
      const float2 v = tab[k.idx];
      const float dv = v.x * u[2 * l] + v.y * u[2 * l + 1];
#pragma unroll
      for (int d = 0; d < 3; ++d) gz[d] += k.dw[d] * dv;
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) gz[d] *= 0.5f;
}

// one value per row (lane = row) -> the B-operand layout: act[b][s] = input
// 4 s + q of row 16 b + r, through the wave's stage st
template <int IN, int SM>
__device__ __forceinline__ void tw_rows_to_b(const float (&v)[IN], float* st, float (&act)[4][SM], int lane) {
  const int q = lane >> 4, r = lane & 15;
#pragma unroll
  for (int k = 0; k < IN; ++k) st[k * MST + lane] = v[k];
  wave_lds_sync();
#pragma unroll
  for (int b = 0; b < 4; ++b) {
#pragma unroll
    for (int s = 0; s < (IN + 3) / 4; ++s) {
      const int k = 4 * s + q;
      act[b][s] = (IN % 4 == 0 || k < IN) ? st[k * MST + 16 * b + r] : 0.f;
    }
  }
  wave_lds_sync();
}

// out = W^T . delta for the layer's weights Wl[H][KI] (row-major, LDS):
// mfma_layer with the A operand read in transposed order.  dl[G][b][g] =
// delta of neuron 16 G + 4 g + q, row 16 b + r (the accumulator layout, which
// is the B operand of K-block 4 G + g); out[GO][b][g] = input 16 GO + 4 g + q
// of the same row.  Inputs past KI are padded with zero weights.
template <int KI, int H>
__device__ __forceinline__ void mfma_layer_t(const float* Wl, const mf4 (&dl)[H / 16][4],
                                             mf4 (&out)[(KI + 15) / 16][4], int q, int r) {
#pragma unroll
  for (int GO = 0; GO < (KI + 15) / 16; ++GO) {
#pragma unroll
    for (int b = 0; b < 4; ++b) out[GO][b] = mf4{0.f, 0.f, 0.f, 0.f};
    const int k = 16 * GO + 4 * (r & 3) + (r >> 2);
    const bool kin = KI % 16 == 0 || k < KI;
#pragma unroll
    for (int s = 0; s < H / 4; ++s) {
      const int j = 4 * s + q;
      const float a = kin ? Wl[j * KI + k] : 0.f;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        out[GO][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, dl[s / 4][b][s % 4], out[GO][b], 0, 0, 0);
    }
  }
}

// The gradients of one layer from its delta (accumulator layout) and the c
// planes of its input (cpl, KC of them): the bias sum_row scale[row]
// delta[row][j] (sb: scale in the layout of dl's rows) into gB, the delta
// planes into the stage st, then dW as a GEMM over the wave's 64 rows into
// gW[H][KC].  MFMA K-block t, lane (q, r) takes row 16 q + t for both
// operands, so a lane reads 16 consecutive floats of one plane.
template <int KC, int H>
__device__ __forceinline__ void tw_layer_grads(const mf4 (&dl)[H / 16][4], const float (&sb)[4], float* st,
                                               const float* cpl, float* gW, float* gB, int q, int r) {
#pragma unroll
  for (int G = 0; G < H / 16; ++G) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float s = 0.f;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        st[(16 * G + 4 * g + q) * MST + 16 * b + r] = dl[G][b][g];
        s += sb[b] * dl[G][b][g];
      }
      s = row_sum16(s);
      if (r == 0) atomicAdd(&gB[16 * G + 4 * g + q], s);
    }
  }
  wave_lds_sync();
#pragma unroll
  for (int GK = 0; GK < (KC + 15) / 16; ++GK) {
    const int k = 16 * GK + r;
    const bool kin = KC % 16 == 0 || k < KC;
    float4 bf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      bf[t] = *reinterpret_cast<const float4*>(&cpl[k * MST + 16 * q + 4 * t]);
      if (!kin) bf[t] = float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int GJ = 0; GJ < H / 16; ++GJ) {
      mf4 d = mf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float4 af = *reinterpret_cast<const float4*>(&st[(16 * GJ + r) * MST + 16 * q + 4 * t]);
        d = __builtin_amdgcn_mfma_f32_16x16x4f32(af.x, bf[t].x, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_16x16x4f32(af.y, bf[t].y, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_16x16x4f32(af.z, bf[t].z, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_16x16x4f32(af.w, bf[t].w, d, 0, 0, 0);
      }
      // D[4 q + g][r] = dW[16 GJ + 4 q + g][16 GK + r]
      if (kin) {
#pragma unroll
        for (int g = 0; g < 4; ++g) atomicAdd(&gW[(16 * GJ + 4 * q + g) * KC + k], d[g]);
      }
    }
  }
  wave_lds_sync();
}

// The forward of the wave's 64 rows from their encodings e: the ReLU mask
// word of every hidden layer, the last hidden layer's activations act (B
// layout) and z = o1 - o0 of the lane's own row.  KEEP: h_l goes to c plane
// 16 + l H + j of cst.
template <int LV, int H, int NL, bool KEEP>
__device__ __forceinline__ float tw_forward(const float* w, const float (&e)[2 * LV], float* st, float* cst,
                                            float (&act)[4][WideShape<LV, H, NL>::SM], uint32_t (&mask)[NL - 1],
                                            int lane) {
  using S = WideShape<LV, H, NL>;
  constexpr int IN = S::IN, NG = S::NG, SM = S::SM;
  const int q = lane >> 4, r = lane & 15;
  tw_rows_to_b<IN, SM>(e, st, act, lane);
  const float* W = w;
#pragma unroll
  for (int layer = 0; layer < NL - 1; ++layer) {
    mf4 acc[NG][4];
    if (layer == 0) mfma_layer<IN, NG, SM>(W, act, acc, q, r);
    else mfma_layer<H, NG, SM>(W, act, acc, q, r);
    const float* B = W + H * (layer == 0 ? IN : H);
    W = B + H;
    uint32_t m = 0;
#pragma unroll
    for (int G = 0; G < NG; ++G) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float bj = B[16 * G + 4 * g + q];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float v = acc[G][b][g] + bj;
          m |= (v > 0.f ? 1u : 0u) << (16 * G + 4 * g + b);
          const float hv = fmaxf(v, 0.f);
          act[b][4 * G + g] = hv;
          if (KEEP) cst[(16 + layer * H + 16 * G + 4 * g + q) * MST + 16 * b + r] = hv;
        }
      }
    }
    mask[layer] = m;
  }
  // output layer: z = (W[1] - W[0]) . h + b1 - b0, summed over this lane's
  // neurons, then over the 4 q lanes of a row; the lane's own row is 16 q + r
  float zp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int G = 0; G < NG; ++G) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j = 16 * G + 4 * g + q;
      const float dw = W[H + j] - W[j];
#pragma unroll
      for (int b = 0; b < 4; ++b) zp[b] += dw * act[b][4 * G + g];
    }
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    zp[b] += __shfl_xor(zp[b], 16, 64);
    zp[b] += __shfl_xor(zp[b], 32, 64);
  }
  const float z = q == 0 ? zp[0] : (q == 1 ? zp[1] : (q == 2 ? zp[2] : zp[3]));
  return z + (W[2 * H + 1] - W[2 * H]);
}

// dz / d(pre-activation of the last hidden layer), accumulator layout
template <int LV, int H, int NL>
__device__ __forceinline__ void tw_delta_z(const float* w, uint32_t m, mf4 (&dl)[H / 16][4], int q) {
  const float* WL = w + WideShape<LV, H, NL>::OL;
#pragma unroll
  for (int G = 0; G < H / 16; ++G) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j = 16 * G + 4 * g + q;
      const float dw = WL[H + j] - WL[j];
#pragma unroll
      for (int b = 0; b < 4; ++b) dl[G][b][g] = mask_bit(m, G, g, b) ? dw : 0.f;
    }
  }
}

// Backward through the hidden layers from dl = delta of the last one down
// to delta_0 (left in dl): delta_{l-1} = up(l - 1, j, b) + D_{l-1} W_l^T
// delta_l.  GRADS: every layer's weight and bias gradients on the way
// (tw_layer_grads, bias scale sb) into the workgroup's gw.
template <int LV, int H, int NL, bool GRADS, class UP>
__device__ __forceinline__ void tw_backward(const float* w, float* gw, const uint32_t (&mask)[NL - 1],
                                            mf4 (&dl)[H / 16][4], const float (&sb)[4], float* st, const float* cst,
                                            UP up, int q, int r) {
  constexpr int IN = 2 * LV, NG = H / 16;
#pragma unroll
  for (int l = NL - 2; l >= 0; --l) {
    const int ow = l == 0 ? 0 : H * IN + H + (l - 1) * (H * H + H);
    if (GRADS) {
      if (l == 0) tw_layer_grads<IN, H>(dl, sb, st, cst, gw, gw + H * IN, q, r);
      else tw_layer_grads<H, H>(dl, sb, st, cst + (16 + (l - 1) * H) * MST, gw + ow, gw + ow + H * H, q, r);
    }
    if (l > 0) {
      mf4 out[NG][4];
      mfma_layer_t<H, H>(w + ow, dl, out, q, r);
#pragma unroll
      for (int G = 0; G < NG; ++G)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            dl[G][b][g] = up(l - 1, 16 * G + 4 * g + q, b) + (mask_bit(mask[l - 1], G, g, b) ? out[G][b][g] : 0.f);
    }
  }
}

// u = W_0^T delta_0, one row per lane
template <int LV, int H>
__device__ __forceinline__ void tw_input_grad(const float* w, const mf4 (&dl)[H / 16][4], float* st,
                                              float (&u)[2 * LV], int lane) {
  const int q = lane >> 4, r = lane & 15;
  mf4 uo[1][4];
  mfma_layer_t<2 * LV, H>(w, dl, uo, q, r);
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int b = 0; b < 4; ++b) st[(4 * g + q) * MST + 16 * b + r] = uo[0][b][g];
  wave_lds_sync();
#pragma unroll
  for (int m = 0; m < 2 * LV; ++m) u[m] = st[m * MST + lane];
  wave_lds_sync();
}

// a row's value (lane = row) in the layout of the accumulator's rows: v[b] = row 16 b + r
__device__ __forceinline__ void tw_row_bcast(float v, float (&vb)[4], int r) {
#pragma unroll
  for (int b = 0; b < 4; ++b) vb[b] = __shfl(v, 16 * b + r, 64);
}

// k_train_norms for a wide shape
template <int LV, int H, int NL>
__global__ void __launch_bounds__(TW_BLOCK)
k_train_norms_wide(NetDev net, const float* __restrict__ xyz, const float* __restrict__ gt, int64_t n, float T,
                   double* __restrict__ stats) {
  using S = WideShape<LV, H, NL>;
  constexpr int IN = S::IN, NW = S::NW;
  __shared__ float w[NW];
  __shared__ __attribute__((aligned(16))) float stg[TW_WAVES * S::DPL * MST];
  for (int i = threadIdx.x; i < NW; i += blockDim.x) w[i] = net.weights[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  float* st = stg + (threadIdx.x >> 6) * (S::DPL * MST);
  const int64_t i = (int64_t)blockIdx.x * TW_BLOCK + threadIdx.x;
  const bool live = i < n;
  float x[3] = {0.5f, 0.5f, 0.5f};
  if (live) load_point(xyz, i, x);
  float e[IN], u[IN], act[4][S::SM];
  uint32_t mask[NL - 1];
  tw_encode<LV>(net, x, e);
  const float z = tw_forward<LV, H, NL, false>(w, e, st, nullptr, act, mask, lane);
  mf4 dl[S::NG][4];
  tw_delta_z<LV, H, NL>(w, mask[NL - 2], dl, q);
  const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
  tw_backward<LV, H, NL, false>(w, nullptr, mask, dl, zero4, st, nullptr, [](int, int, int) { return 0.f; }, q, r);
  tw_input_grad<LV, H>(w, dl, st, u, lane);
  float gz[3];
  tw_encode_dx<LV>(net, x, u, gz);
  const float y = tanhf(z);
  const float ty = 1.f - y * y;
  double l1 = 0.0, j2 = 0.0;
  if (live) {
    l1 = fabsf(clamp_t(y, T) - clamp_t(gt[i], T));
#pragma unroll
    for (int d = 0; d < 3; ++d) j2 += (double)(ty * gz[d]) * (ty * gz[d]);
  }
  l1 = tnp::wave_sum(l1);
  j2 = tnp::wave_sum(j2);
  if (lane == 0) {
    atomicAdd(&stats[0], l1);
    atomicAdd(&stats[1], j2);
  }
}

// k_train_grads (its three modes) for a wide shape
template <int LV, int H, int NL>
__global__ void __launch_bounds__(TW_BLOCK)
k_train_grads_wide(NetDev net, const float* __restrict__ xyz, const float* __restrict__ gt, int64_t n, float T,
                   float eik_w, int64_t eik_batch, const double* __restrict__ stats, float* __restrict__ g_table,
                   float* __restrict__ g_w, const float* __restrict__ gout, const float* __restrict__ gJ,
                   float* __restrict__ g_x) {
  using S = WideShape<LV, H, NL>;
  constexpr int IN = S::IN, NH = S::NH, NG = S::NG, NW = S::NW, SM = S::SM;
  __shared__ float w[NW];
  __shared__ float gw[NW];
  __shared__ __attribute__((aligned(16))) float stg[TW_WAVES * (S::DPL + S::CPL) * MST];
  for (int i = threadIdx.x; i < NW; i += blockDim.x) {
    w[i] = net.weights[i];
    gw[i] = 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  float* st = stg + (threadIdx.x >> 6) * ((S::DPL + S::CPL) * MST);
  float* cst = st + S::DPL * MST;
  const int64_t i = (int64_t)blockIdx.x * TW_BLOCK + threadIdx.x;
  const bool live = i < n;
  float x[3] = {0.5f, 0.5f, 0.5f};
  if (live) load_point(xyz, i, x);
  float e[IN], u[IN];
  uint32_t mask[NH];
  float gz[3], y;
  {
    float act[4][SM];
    tw_encode<LV>(net, x, e);
    y = tanhf(tw_forward<LV, H, NL, true>(w, e, st, cst, act, mask, lane));
  }
  const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
  auto no_up = [](int, int, int) { return 0.f; };
  {
    mf4 dl[NG][4];
    tw_delta_z<LV, H, NL>(w, mask[NH - 1], dl, q);
    tw_backward<LV, H, NL, false>(w, nullptr, mask, dl, zero4, st, nullptr, no_up, q, r);
    tw_input_grad<LV, H>(w, dl, st, u, lane);
  }
  tw_encode_dx<LV>(net, x, u, gz);
  const float ty = 1.f - y * y;
  float v[3] = {0.f, 0.f, 0.f};
  if (gJ) {
    if (live)
#pragma unroll
      for (int d = 0; d < 3; ++d) v[d] = gJ[3 * i + d];
  } else if (!gout) {
    // v_i = c J_i (train_net.h k_train_grads)
    const double nj = sqrt(stats[1]);
    const float c = nj > 0.0 ? (float)(eik_w * 2.0 * (nj - 1.0) / ((double)eik_batch * nj)) : 0.f;
#pragma unroll
    for (int d = 0; d < 3; ++d) v[d] = c * ty * gz[d];
  }
  const float qv = v[0] * gz[0] + v[1] * gz[1] + v[2] * gz[2];
  float rho = 0.f;
  if (!gout && !gJ && live && y >= -T && y <= T) {
    const float rr = clamp_t(y, T) - clamp_t(gt[i], T);
    rho = (rr > 0.f ? 1.f : (rr < 0.f ? -1.f : 0.f)) / (float)n;
  }
  const float kappa = !live ? 0.f : (gout ? ty * gout[i] : ty * (rho - 2.f * y * qv));
  const float mu = (live && !gout) ? ty : 0.f;
  // per lane as in k_train_grads: the direction a, the table terms, the Hessian term
  const float2* tab = reinterpret_cast<const float2*>(net.table);
  float a[IN];
  float hz[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int l = 0; l < LV; ++l) {
    float t[3];
    uint32_t g[3];
    tcell_of(net, l, x, t, g);
    const float s = net.scales[l];
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) {
      const TCorner k = tcorner_of(net, l, t, g, cc);
      const float gv = 0.5f * (k.dw[0] * v[0] + k.dw[1] * v[1] + k.dw[2] * v[2]);
      const float2 e2 = tab[k.idx];
      s0 += e2.x * gv;
      s1 += e2.y * gv;
      const float coef = kappa * k.w + mu * gv;
      if (live && coef != 0.f) {
        if (u[2 * l] != 0.f) unsafeAtomicAdd(&g_table[2 * (size_t)k.idx], u[2 * l] * coef);
        if (u[2 * l + 1] != 0.f) unsafeAtomicAdd(&g_table[2 * (size_t)k.idx + 1], u[2 * l + 1] * coef);
      }
      if (g_x) {
        const float tu = e2.x * u[2 * l] + e2.y * u[2 * l + 1];
#pragma unroll
        for (int qd = 0; qd < 3; ++qd) {
          float hv = 0.f;
#pragma unroll
          for (int rd = 0; rd < 3; ++rd) {
            if (rd == qd) continue;
            const int od = 3 - qd - rd;
            const float sq = ((cc >> qd) & 1) ? 1.f : -1.f, sr = ((cc >> rd) & 1) ? 1.f : -1.f;
            hv += sq * sr * s * s * k.f[od] * v[rd];
          }
          hz[qd] += tu * hv;
        }
      }
    }
    a[2 * l] = s0;
    a[2 * l + 1] = s1;
  }
  if (g_x && live) {
#pragma unroll
    for (int d = 0; d < 3; ++d) g_x[3 * i + d] += ty * 0.25f * hz[d] - 2.f * y * ty * qv * gz[d];
  }
  // c_{-1} = kappa e + mu a, one row per lane
#pragma unroll
  for (int m = 0; m < IN; ++m) cst[m * MST + lane] = kappa * e[m] + mu * a[m];
  float kb[4], mb[4];
  tw_row_bcast(kappa, kb, r);
  tw_row_bcast(mu, mb, r);
  // tangent pass h'_l = D_l W_l h'_{l-1} (no bias), c_l = kappa h_l + mu h'_l
  // in place of h_l; the last c is the output layer's weight gradient
  {
    float act[4][SM];
    tw_rows_to_b<IN, SM>(a, st, act, lane);
    const float* W = w;
#pragma unroll
    for (int layer = 0; layer < NH; ++layer) {
      mf4 acc[NG][4];
      if (layer == 0) mfma_layer<IN, NG, SM>(W, act, acc, q, r);
      else mfma_layer<H, NG, SM>(W, act, acc, q, r);
      W += H * (layer == 0 ? IN : H) + H;
#pragma unroll
      for (int G = 0; G < NG; ++G) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int j = 16 * G + 4 * g + q;
          float cs = 0.f;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const float hp = mask_bit(mask[layer], G, g, b) ? acc[G][b][g] : 0.f;
            act[b][4 * G + g] = hp;
            float* cp = &cst[(16 + layer * H + j) * MST + 16 * b + r];
            const float c = kb[b] * *cp + mb[b] * hp;
            *cp = c;
            cs += c;
          }
          if (layer == NH - 1) {
            cs = row_sum16(cs);
            if (r == 0) {
              atomicAdd(&gw[S::OL + j], -cs);
              atomicAdd(&gw[S::OL + H + j], cs);
            }
          }
        }
      }
    }
  }
  const float ks = tnp::wave_sum(kappa);
  if (lane == 0) {
    atomicAdd(&gw[S::OL + 2 * H], -ks);
    atomicAdd(&gw[S::OL + 2 * H + 1], ks);
  }
  wave_lds_sync();
  // delta again, layer by layer, with every layer's gradients
  {
    mf4 dl[NG][4];
    tw_delta_z<LV, H, NL>(w, mask[NH - 1], dl, q);
    tw_backward<LV, H, NL, true>(w, gw, mask, dl, kb, st, cst, no_up, q, r);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < NW; k += blockDim.x)
    if (gw[k] != 0.f) unsafeAtomicAdd(&g_w[k], gw[k]);
}

// k_forward_vjp for a wide shape
template <int LV, int H, int NL>
__global__ void __launch_bounds__(TW_BLOCK)
k_forward_vjp_wide(NetDev net, const float* __restrict__ xyz, int64_t n, const float* __restrict__ gpl, int64_t ld,
                   const float* __restrict__ gout2, float* __restrict__ g_table, float* __restrict__ g_w,
                   float* __restrict__ g_x) {
  using S = WideShape<LV, H, NL>;
  constexpr int IN = S::IN, NH = S::NH, NG = S::NG, NW = S::NW, SM = S::SM;
  __shared__ float w[NW];
  __shared__ float gw[NW];
  __shared__ __attribute__((aligned(16))) float stg[TW_WAVES * (S::DPL + S::CPL) * MST];
  for (int i = threadIdx.x; i < NW; i += blockDim.x) {
    w[i] = net.weights[i];
    gw[i] = 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  float* st = stg + (threadIdx.x >> 6) * ((S::DPL + S::CPL) * MST);
  float* cst = st + S::DPL * MST;
  const int64_t i = (int64_t)blockIdx.x * TW_BLOCK + threadIdx.x;
  const int64_t i0 = i - lane;  // the wave's first row
  const bool live = i < n;
  float x[3] = {0.5f, 0.5f, 0.5f};
  if (live) load_point(xyz, i, x);
  float e[IN], de[IN];
  uint32_t mask[NH];
  float act[4][SM];
  tw_encode<LV>(net, x, e);
  tw_forward<LV, H, NL, true>(w, e, st, cst, act, mask, lane);  // c_l = h_l
#pragma unroll
  for (int m = 0; m < IN; ++m) cst[m * MST + lane] = e[m];  // c_{-1} = e
  // upstream of plane p at row 16 b + r of this wave
  auto up_at = [&](int p, int b) {
    const int64_t row = i0 + 16 * b + r;
    return (gpl && row < n) ? gpl[(int64_t)p * ld + row] : 0.f;
  };
  // output layer: o = WL h + bL; the gathered o1 - o0 adds (-g, +g)
  const float gl = (live && gpl) ? gpl[(int64_t)(NH * H) * ld + i] : 0.f;
  float go[2] = {-gl, gl};
  if (live && gout2) {
    go[0] += gout2[2 * i];
    go[1] += gout2[2 * i + 1];
  }
  if (!live) go[0] = go[1] = 0.f;
  float g0[4], g1[4];
  tw_row_bcast(go[0], g0, r);
  tw_row_bcast(go[1], g1, r);
  const float* WL = w + S::OL;
  mf4 dl[NG][4];
#pragma unroll
  for (int G = 0; G < NG; ++G) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j = 16 * G + 4 * g + q;
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        s0 += g0[b] * act[b][4 * G + g];
        s1 += g1[b] * act[b][4 * G + g];
        const float dh = g0[b] * WL[j] + g1[b] * WL[H + j];
        dl[G][b][g] = up_at((NH - 1) * H + j, b) + (mask_bit(mask[NH - 1], G, g, b) ? dh : 0.f);
      }
      s0 = row_sum16(s0);
      s1 = row_sum16(s1);
      if (r == 0) {
        atomicAdd(&gw[S::OL + j], s0);
        atomicAdd(&gw[S::OL + H + j], s1);
      }
    }
  }
  const float b0 = tnp::wave_sum(go[0]), b1 = tnp::wave_sum(go[1]);
  if (lane == 0) {
    atomicAdd(&gw[S::OL + 2 * H], b0);
    atomicAdd(&gw[S::OL + 2 * H + 1], b1);
  }
  wave_lds_sync();
  const float one4[4] = {1.f, 1.f, 1.f, 1.f};  // dead rows have a zero delta
  tw_backward<LV, H, NL, true>(w, gw, mask, dl, one4, st, cst,
                               [&](int l, int j, int b) { return up_at(l * H + j, b); }, q, r);
  tw_input_grad<LV, H>(w, dl, st, de, lane);
  // the encoding: table terms and d/dx
  float gxd[3];
  tw_encode_dx<LV>(net, x, de, gxd);
#pragma unroll
  for (int l = 0; l < LV; ++l) {
    float t[3];
    uint32_t g[3];
    tcell_of(net, l, x, t, g);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const TCorner k = tcorner_of(net, l, t, g, c);
      if (live && k.w != 0.f) {
        if (de[2 * l] != 0.f) unsafeAtomicAdd(&g_table[2 * (size_t)k.idx], k.w * de[2 * l]);
        if (de[2 * l + 1] != 0.f) unsafeAtomicAdd(&g_table[2 * (size_t)k.idx + 1], k.w * de[2 * l + 1]);
      }
    }
  }
  if (g_x && live)
#pragma unroll
    for (int d = 0; d < 3; ++d) g_x[3 * i + d] += gxd[d];
  __syncthreads();
  for (int k = threadIdx.x; k < NW; k += blockDim.x)
    if (gw[k] != 0.f) unsafeAtomicAdd(&g_w[k], gw[k]);
}

}  // namespace
