// gate4_kernel: the WN gate conv of SHORT calls on 64-row x 12-column workgroups with the 4x4x1 MFMA.
// (gfx950 / CDNA4 device code; reference arithmetic: modules.py:196-199 -- x_in = in_layers[i](x); acts =
// fused_add_tanh_sigmoid_multiply(x_in, g_l) (commons.py:99-106); paths relative to /root/reference/src/python/piper_train/vits/.)
#pragma once
#include "conv_common.h"

namespace pe {

// conv_splitk16_kernel<true, 12, 2> gives one utterance's gate conv (384 x 960 x 417) 27 column tiles x 6 channel groups =
// 162 workgroups -- 162 of 256 CUs, each matrix-pipe bound for 3.8 us (960 16x16x4 MFMAs on SIMDs that three waves share).
// The 16-column tile is the 16x16x4 MFMA's; v_mfma_f32_4x4x1 (64 rows x 4 columns per instruction at the same MAC rate)
// allows 12: 35 x 6 = 210 workgroups with 0.75x the matrix time each.
//   * workgroup = one 32-channel group = 64 GEMM rows (lane l < 32: the tanh row of channel 32 g + l, l >= 32: the sigmoid
//     row of channel 32 g + l - 32) x 12 output columns x K = 192 channels x ntaps (<= 5, dilation 1);
//   * 12 waves: wave w owns input channels [16 w, 16 w + 16) for every tap and all three 4-column groups: 20 16-byte
//     weight loads per lane (all in flight at kernel entry, behind the 4 window loads) and 240 MFMAs, three independent
//     accumulator chains; B operand = the x window, transposed in LDS ([16 columns][192 + 4]: a lane reads four channel
//     steps of its column as one 16-byte LDS read, a tap is the next row);
//   * the twelve partial tiles meet in LDS in wave order (deterministic), then bias + speaker bias + tanh * sigmoid.
// Weights: engine_pack.cpp pack_gate4 -- [group][tap][k quad 48][lane][4].
constexpr int G4_NC = 12, G4_WC = 16, G4_NW = 12, G4_K = 192, G4_XS = G4_K + 4;
// The same conv with the coupling layer's `pre` (1x1, 96 -> 192; modules.py:433, 455) composed into it when the weights are
// packed (engine_pack.cpp pack_gate4pre): Wc_k = Wg_k . Wp over the 96 channels of x0 -- K = 96 x ntaps, 6 waves, half the
// weight stream and half the MFMAs. gate4pre_kernel below; everything else is gate4_kernel's.
//   * pre's bias reaches the gate conv only through taps whose input column lies inside [0, L): h = pre(x0) . mask is zero
//     outside. B_k = Wg_k . b_pre per tap; `tapb` = [ntaps rows B_k | row 5: the gate conv's own bias][2 x split]. A
//     workgroup none of whose columns has a tap outside [0, L) adds p.bias = b_gate + sum_k B_k (rounded once from f64);
//     the others (wave-uniform branch) add b_gate + B_k over the inside taps, in tap order. Then the speaker bias, as ever.
constexpr int G4P_K = 96, G4P_NW = G4P_K / 16;
// Kernel entry (pe_rt.h PE_ENTRY_BATCH): everything in front of the loads arrives in SGPRs (13 dwords; gate4pre_kernel:
// 14, Cin is the constant 96 there and tapb rides along); the leading parameters repeat p's fields of the same names.
template <int K>
__device__ __forceinline__ void gate4_body(ConvP& p, const float* tapb) {
  constexpr int NW = K / 16, XS = K + 4;
  PE_DYN_SMEM(float, sm);                         // XT[16][K + 4] | P[K / 16 waves][64][12]
  float* XT = sm;
  float* P = XT + G4_WC * XS;
  const int b = blockIdx.z, grp = blockIdx.y;
  PE_STAMP(5, 0);
  const int L = p.lens[b] * p.len_mul;            // first used after every load below is requested
  const int n0 = blockIdx.x * G4_NC;
  const int tid = threadIdx.x, lane = tid & 63, wv = PE_UNIFORM(tid >> 6);
  const int l3 = lane & 3, lb = lane >> 2;
  const int ntaps = p.ntaps;
  // ---- the x window (K channels x 16 columns from n0 - padl), then this wave's fragments
  const pe_rowsrc xd = pe_make_row(p.x + (long)b * p.x_bs, p.Cin * p.x_cs);
  float xv[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = tid + 64 * NW * u, ch = idx >> 4, c = idx & 15, t = n0 - p.padl + c;
    xv[u] = pe_row_load(xd, (t >= 0 && t < p.x_cs) ? ch * p.x_cs + t : -1);
  }
  PE_SCHED_FENCE();
  f32x4 wf[5][4];
  {
    const int tap_floats = (K / 4) * 256;       // one tap of one group: 48 quads x 64 lanes x 4
    const pe_rowsrc wd = pe_make_row_u(p.wpg4 + (long)grp * ntaps * tap_floats, ntaps * tap_floats);
#pragma unroll
    for (int tp = 0; tp < 5; ++tp)
#pragma unroll
      for (int q = 0; q < 4; ++q) wf[tp][q] = pe_row_load4(wd, tp < ntaps ? ((tp * (K / 4) + 4 * wv + q) * 64 + lane) * 4 : -4);
  }
  PE_SCHED_FENCE();
  if (n0 >= L) return;
  PE_STAMP(5, 1);
  {
    const float slope = p.in_slope;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = tid + 64 * NW * u, ch = idx >> 4, c = idx & 15, t = n0 - p.padl + c;
      float v = (t < L) ? xv[u] : 0.f;               // (t < 0: the load was poisoned)
      if (slope != 1.f) v = pe_lrelu(v, slope);
      XT[c * XS + ch] = v;
    }
  }
  __syncthreads();
  PE_STAMP(5, 2);
  // ---- this wave's partial tile over its 16 channels x ntaps
  {
    f32x4 acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[g][r] = 0.f;
    const float* xp = XT + l3 * XS + 16 * wv;
#pragma unroll
    for (int tp = 0; tp < 5; ++tp) {
      if (tp < ntaps) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 b4[3];
#pragma unroll
          for (int g = 0; g < 3; ++g) b4[g] = *reinterpret_cast<const f32x4*>(xp + (4 * g + tp) * XS + 4 * q);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = pe_mfma_4x4x1(wf[tp][q][j], b4[g][j], acc[g]);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) P[(wv * 64 + 4 * lb + r) * G4_NC + 4 * g + l3] = acc[g][r];
  }
  PE_STAMP(5, 3);
  __syncthreads();
  PE_STAMP(5, 4);
  // ---- the twelve partial tiles in wave order, biases, tanh * sigmoid (commons.py:99-106)
  if (tid < 32 * G4_NC) {
    const int c = tid / G4_NC, col = tid - c * G4_NC;
    const int ch = grp * 32 + c, t = n0 + col;
    if (ch < p.split && t < L) {
      float ta = 0.f, sa = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        ta += P[(w * 64 + c) * G4_NC + col];
        sa += P[(w * 64 + 32 + c) * G4_NC + col];
      }
      if constexpr (K == G4P_K) {
        // pre's bias through the taps inside [0, L) (see above); conv_store_gate's additions in its order otherwise
        float bt = p.bias[ch], bs = p.bias[p.split + ch];
        if (PE_UNIFORM(n0 < p.padl || n0 + G4_NC + ntaps - 1 - p.padl > L)) {
          const int rs = 2 * p.split;
          bt = tapb[5 * rs + ch];
          bs = tapb[5 * rs + p.split + ch];
          for (int k = 0; k < ntaps; ++k) {
            const int u = t + k - p.padl;
            if (u >= 0 && u < L) { bt += tapb[k * rs + ch]; bs += tapb[k * rs + p.split + ch]; }
          }
        }
        ta += bt;
        sa += bs;
        if (p.bias2) {
          const float* b2 = p.bias2 + (long)b * p.bias2_bs;
          ta += b2[ch];
          sa += b2[p.split + ch];
        }
        p.out[(long)b * p.o_bs + (long)ch * p.o_cs + t] = tanhf(ta) * (1.f / (1.f + expf(-sa)));
      } else {
        conv_store_gate(p, b, ch, t, ta, sa);
      }
    }
  }
  PE_STAMP(5, 5);
}

__global__ __launch_bounds__(64 * G4_NW) void gate4_kernel(const int* lens, int len_mul, const float* x, long x_bs, int x_cs,
                                                           int Cin, int padl, int ntaps_, const float* wpg4, ConvP p) {
  PE_KTRACE(4);
  p.lens = lens; p.len_mul = len_mul; p.x = x; p.x_bs = x_bs; p.x_cs = x_cs; p.Cin = Cin; p.padl = padl; p.ntaps = ntaps_;
  p.wpg4 = wpg4;
  gate4_body<G4_K>(p, nullptr);
}
// x = the 96 channels of x0 inside the latent (p.Cin == 96), wpg4 = the composed matrix, [group][tap][k quad 24][lane][4]
__global__ __launch_bounds__(64 * G4P_NW) void gate4pre_kernel(const int* lens, int len_mul, const float* x, long x_bs, int x_cs,
                                                               int padl, int ntaps_, const float* wpg4, const float* tapb, ConvP p) {
  PE_KTRACE(4);
  p.lens = lens; p.len_mul = len_mul; p.x = x; p.x_bs = x_bs; p.x_cs = x_cs; p.Cin = G4P_K; p.padl = padl; p.ntaps = ntaps_;
  p.wpg4 = wpg4;
  gate4_body<G4P_K>(p, tapb);
}

}  // namespace pe
