// One launcher per kernel family: parameter structs, grids, shared-memory sizes, profile rows; which form a launch takes is
// asked of the launch policy (policy.h) -- for the convs once per launch, in plan_conv.
#include "engine_internal.h"

namespace pe {

// ------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------

static int tile_cfg_of(int cfg) { return cfg == CFG_C ? CFG_C : CFG_S; }      // non-gate configurations: 32 x 128 or 64 x 64 tiles
static int slab_halo(int xhalo) { return xhalo <= 64 ? 64 : 128; }
// dynamic LDS: the tiled kernels' nbuf slabs of KC channels x (BN + halo) columns; the split-K kernels' KC x xw slab per wave, or the waves' partial tiles
static size_t tile_smem(int nbuf, int BN, int halo) { return (size_t)nbuf * KC * ((BN + halo + 63) / 64 * 64) * sizeof(float); }
static size_t splitk_smem(int nw, int MT, int xw) { return std::max<size_t>((size_t)nw * KC * xw, (size_t)nw * MT * 16 * 64) * sizeof(float); }

// Where a conv launch is decided: policy.h answers the questions, this function asks them once.
ConvPlan Engine::plan_conv(const PackedConv& pc, int Lmax, int epi, bool stage_tiled) const {
  ConvPlan pl;
  const bool convt = epi == EPI_CONVT;
  const int ncols = pl.ncols = convt ? Lmax + 1 : Lmax;
  const int xhalo = (pc.ntaps - 1) * pc.dil, units = pc.nchunks * pc.ntaps;
  // (the thresholds are asked with the PACKED configuration's tile count, whatever configuration is launched below)
  pl.blocks = tile_workgroups(CFG_BM[pc.cfg], CFG_BN[pc.cfg], ncols, pc.mtiles, B_);
  pl.halo = slab_halo(xhalo);
  const bool to_splitk = !stage_tiled && pol_.splitk(pl.blocks, xhalo, pc.Cin);
  const bool direct = pol_.one_tap_direct(pc.gate, convt, pc.ntaps, pc.Cin);
  // A conv that may ride in a grouped split-K launch: few enough column tiles that the launch is latency- rather than
  // throughput-bound, and a halo the 128-column slab covers. The tiled kernel's grouped form: a plain conv (no gate, no
  // ConvTranspose) that takes the tiled route anyway.
  pl.group_splitk = !stage_tiled && !convt && pol_.groupable(pc.gate, pc.up != 0, pl.blocks, xhalo, pc.Cin);
  pl.group_tiled = !pc.gate && pc.up == 0 && !convt && !to_splitk && !(matrix_bf3_ && pc.wpb) && !direct && xhalo <= 128;
  pl.group_cfg = tile_cfg_of(pc.cfg);
  if (to_splitk && epi == EPI_GATE &&
      pol_.gate_12col(pc.gate, pc.wpg4 != nullptr && pc.Cin == 192, pc.ntaps, pc.dil, tile_workgroups(32, 12, ncols, pc.split / 32, B_))) {
    // the WN gate conv of a short call: 64 rows x 12 columns per workgroup on the 4x4x1 MFMA (kernels/gate4.h)
    pl.form = CONV_GATE12;
    pl.grid = dim3((ncols + 11) / 12, pc.split / 32, B_);
    pl.smem = ((size_t)16 * 196 + (size_t)12 * 64 * 12) * sizeof(float);
    return pl;
  }
  if (to_splitk) {
    // few columns (one utterance through encoder / duration predictor / flow): split K across the waves
    // waves per workgroup: 4 / 8 take whole chunks; the WN gate conv (6 chunks x 5 taps, two M tiles per wave)
    // goes to 12 waves whose two halves split the taps: 15.8 -> 14.2 us per launch at B=1. Measured and not used:
    // the same 12 waves for conv_pre (6 x 7) and FFN conv_2 (24 chunks) are slower than 8.
    pl.form = CONV_SPLITK;
    pl.MT = pc.gate ? 2 : 1;
    pl.nw = pc.nchunks >= 5 ? 8 : 4;
    if (pol_.splitk_12wave(pc.gate, units, pc.nchunks, pc.ntaps)) {
      pl.nw = 12;
      pl.tgroups = pc.nchunks <= 6 ? 2 : 1;
    }
    pl.grid = dim3((ncols + 31) / 32, pc.mtiles / pl.MT, B_);
    pl.smem = splitk_smem(pl.nw, pl.MT, 64);
    // MFMA-pipe bound inside the workgroup (>= 24 chunk-tap units) although most CUs idle: 16 output columns
    if (pol_.splitk_16col(pc.wp16 != nullptr, convt, pc.gate, units)) {
      pl.form = CONV_SPLITK16;
      pl.grid.x = (ncols + 15) / 16;
      // the gate conv of a SHORT utterance (<= 128 workgroups of 12 waves: half the CUs idle): half a channel group per
      // workgroup on 6 waves (one chunk and every tap each, all five weight steps in flight at entry) is twice the
      // workgroups with half the matrix time each -- 64 ids: 9.64 -> 8.37 us per launch; beyond one workgroup per CU it
      // loses (128 ids, 324 workgroups: 9.77 -> 12.6 us; profiles/r04_notes.md, call 32)
      pl.half = pol_.gate_half_groups(pc.gate, pc.nchunks, pc.ntaps, tile_workgroups(32 * pl.MT, 16, ncols, pc.mtiles, B_));
      if (pl.half) pl.grid.y *= 2;
      pl.nw = pc.gate ? (pl.half ? 6 : 12) : 8;
      pl.tgroups = pc.gate ? (pl.half ? 1 : (pc.nchunks <= 6 ? 2 : 1)) : 1;
      pl.smem = (size_t)pl.nw * KC * 64 * sizeof(float);
    }
    return pl;
  }
  // polyphase up-conv: a lane's four accumulator rows are consecutive output samples of one channel (stride a multiple of
  // 4) or both phases of two channels (stride 2): stored as 16- / 8-byte pieces straight from the accumulators (the 32x32
  // result layout of the tiled f32 kernel and of the split-operand kernel is the same). Measured against one 4-byte store
  // per phase and against the tile transposed through LDS (profiles/r04_notes.md, calls 7 / 11).
  pl.up_vec = (convt && pol_.convt_vec) ? (pc.up % 4 == 0 ? 4 : (pc.up == 2 ? 2 : 0)) : 0;
  if (matrix_bf3_ && pc.wpb && xhalo <= 128) {
    // split matrix modes (bf16x3 / f16x3 / bf16x6): 128 x 128 / 64 x 128 / 32 x 256 tiles (two 32x32 MFMA tiles per wave at least: the bf16 pipe
    // is fast enough that operand traffic per MFMA matters more than workgroup count)
    static const int BF3_BM[] = {128, 64, 32}, BF3_BN[] = {128, 128, 256};
    const int bc = pl.cfg = pc.cfg == CFG_A ? 0 : (pc.cfg == CFG_B ? 1 : 2);
    if (pc.gate && bc == 2) throw std::runtime_error("internal: gate conv packed for 32-row blocks");
    pl.form = CONV_SPLIT;
    pl.nbuf = pc.nchunks == 1 ? 1 : 2;
    const int nterm = matrix_sm_ == 2 ? 3 : 2;
    pl.smem = (size_t)pl.nbuf * nterm * 64 * ((BF3_BN[bc] + pl.halo + 63) / 64 * 64);       // [terms][4 k groups][XS] x 16 B
    pl.grid = dim3((ncols + BF3_BN[bc] - 1) / BF3_BN[bc], pc.mtiles * 32 / BF3_BM[bc], B_);
    return pl;
  }
  if (direct) {
    // one tap: nothing to share between the MFMA's k rows, so the B operand skips LDS (kernels/conv1x1.h)
    pl.form = CONV_1X1;
    pl.grid = dim3((ncols + 63) / 64, (pc.mtiles + 1) / 2, B_);
    return pl;
  }
  // 32x32 wave tiles everywhere (64x64 / 32x128 workgroup tiles; the gate form pairs two row tiles per wave): measured in
  // rounds 1-3 against 128x128, 64x128 and 256-column tiles at every batch size -- latency here is hidden across
  // workgroups, occupancy beats register reuse (profiles/r01_ablation.txt, r02_notes.md); the larger instantiations are gone
  pl.cfg = pc.cfg == CFG_A ? (pc.gate ? CFG_G : CFG_S) : ((pc.cfg == CFG_B && !pc.gate) ? CFG_S : pc.cfg);
  const int BM = CFG_BM[pl.cfg], BN = CFG_BN[pl.cfg];
  // Column tiles walked by one workgroup. Measured on MI355X (profiles/r01_tpb_sweep.txt): with 2-3
  // workgroups resident per CU, one tile per workgroup (latency hidden across workgroups) beats walking
  // several tiles with the in-kernel prefetch pipeline at every batch size, so the default is 1; the
  // multi-tile path stays available through PIPER_HIP_TPB.
  pl.tpb = pol_.tiles_per_workgroup();
  pl.grid = dim3(((ncols + BN - 1) / BN + pl.tpb - 1) / pl.tpb, pc.mtiles * 32 / BM, B_);
  if (xhalo > 128) throw std::runtime_error("conv halo (kernel-1)*dilation > 128 is not supported");
  // one x slab when the workgroup only ever stages one (single chunk, single tile): more workgroups per CU
  pl.nbuf = (pl.tpb == 1 && pc.nchunks == 1) ? 1 : 2;
  pl.smem = tile_smem(pl.nbuf, BN, pl.halo);
  return pl;
}

// The level-2 profile row of a planned launch: the instantiation exactly as rocprofv3 prints it (minus spaces), as
// kernels/launch_conv.cpp / launch_bf3.cpp pick it from the same plan (tests/test_launch_plan_emu.py holds the two together).
// PIPER_HIP_PROF_SITES=1 (tuning aid): one row per conv SHAPE of the tiled and one-tap kernels instead.
static std::string conv_row_name(const ConvPlan& pl, const PackedConv& pc, int sm, bool sites, int epi, int len_mul) {
  static const char* knames[] = {"2,2,2,2,8", "1,4,2,1,16", "1,4,1,1,16", "2,2,1,1,16", "2,2,2,1,16", "1,4,1,2,16", "1,4,2,2,8"};
  static const char* bnames[] = {"2,2,2,2", "2,2,1,2", "1,4,1,2"};
  const char* g = pc.gate ? "true" : "false";
  char nm[96];
  int n = 0;
  switch (pl.form) {
    case CONV_GATE12: return "gate4_kernel";
    case CONV_SPLITK:
      snprintf(nm, sizeof(nm), "conv_splitk_kernel<%d,%s,%d,%d>", pl.MT, g, pl.nw, pc.gate ? (pl.nw == 12 ? 2 : 3) : 4);
      break;
    case CONV_SPLITK16:      // (the default GT = 4 included)
      snprintf(nm, sizeof(nm), "conv_splitk16_kernel<%s>", pc.gate ? (pl.half ? "true,6,5,2" : "true,12,2,4") : "false,8,4,4");
      break;
    case CONV_SPLIT:
      snprintf(nm, sizeof(nm), "conv_split_kernel<%d,%s,%s,%d>", sm, (pc.gate && pl.cfg == 1) ? "1,4,2,1" : bnames[pl.cfg], g, pl.halo);
      break;
    case CONV_1X1:
      n = snprintf(nm, sizeof(nm), "conv1x1_kernel<1>");
      if (sites) snprintf(nm + n, sizeof(nm) - n, "|%dx%dx%d e%d L%d", pc.rows, pc.Cin, pc.ntaps, epi, len_mul);
      break;
    case CONV_TILE:
      n = snprintf(nm, sizeof(nm), "conv_mfma_kernel<%s,%s,%d>", knames[pl.cfg], g, pl.halo);
      if (sites) snprintf(nm + n, sizeof(nm) - n, "|%dx%dx%d d%d e%d L%d", pc.rows, pc.Cin, pc.ntaps, pc.dil, epi, len_mul);
      break;
  }
  return nm;
}

// How the resblocks of a generator stage are issued, and the only place that decides whether the stage keeps the tiled
// kernel. One launch per stage (mrf_kernel). Measured (profiles/r03_notes.md): ResBlock2 stages (medium / x-low) win at every
// batch size (B=1 -3 %, B=16 / 64 +4.5 % end to end over the conv-by-conv schedule); ResBlock1 stages (high) tie at
// one utterance and lose at batch (its 64-channel stage: 86 vs ~110 TFLOP/s for the conv GEMM kernel on K = 64 * 11
// convs), so those are fused for one or two utterances and on 32 channels only.
// (split matrix modes: the two-term modes run the fused stage on the 16-bit pipe, mrf_split_kernel; mode bf16x6 keeps the f32
// fused kernel for a few utterances and goes conv by conv on the 16-bit pipe from PIPER_HIP_BF3_MINF frames up)
// Grouped sibling launches are a single-utterance latency measure: measured -24 us (medium) / -4 % (high) at B=1, but
// +1..2 % at B=2 and B=4, where every conv already fills the chip on its own; the same schedule goes through the TILED
// kernel where one conv of the stage is only a few tiles per CU (the high voice's 128- / 64-channel stages of a single
// utterance: 834 tiles = 3.26 per CU).
Engine::StageSchedule Engine::stage_schedule(const UpStage& st, int Lmax, double fsum, bool buffers_fit) const {
  if (pol_.mrf_stage(st.mrf_ok, st.mrf_rb1, st.mrf_cp, fsum, matrix_bf3_, matrix_bf3_ && pol_.mrf_split && st.mrf_wsplit != nullptr))
    return {STAGE_FUSED, false};
  const int nk = arch_[A_NRB];
  const long blocks64 = tile_workgroups(64, 64, Lmax, rup(st.ch, 64) / 32, B_);
  const bool tiled = pol_.stage_all_tiled(B_, nk, blocks64);
  const PackedConv& c0 = st.rb[0][0];
  const int tc = tile_cfg_of(c0.cfg);
  bool grp = pol_.group_stage(B_, nk, blocks64, buffers_fit);
  bool grp_t = pol_.group_stage_tiled(nk, tile_workgroups(CFG_BM[tc], CFG_BN[tc], Lmax, rup(c0.rows, CFG_BM[tc]) / 32, B_), buffers_fit);
  for (auto& cv : st.rb) {
    if (cv.size() != st.rb[0].size()) grp = grp_t = false;
    for (auto& c : cv) {
      const ConvPlan pl = plan_conv(c, Lmax, EPI_STORE, tiled);
      grp = grp && pl.group_splitk;
      grp_t = grp_t && pl.group_tiled && pl.group_cfg == tc;
    }
  }
  return {grp ? STAGE_GROUP_SPLITK : (grp_t ? STAGE_GROUP_TILED : STAGE_CHAIN), tiled};
}

// Where the coupling flow's route is decided: what the weights allow was settled at pack time (Rcl's *_ok flags), the policy
// answers for the knobs and the call's size, this function asks once per call.
// Small calls: the LAST WN layer's res/skip conv (skip rows only) rides in front of the post + pre chain launch. Where the
// chain is 4 columns wide and the gate conv runs on gate4_kernel, pre is composed into the first gate conv (gate4pre_kernel
// reads x0; nobody computes h = pre(x0) in front of the WN -- the first res/skip launch writes h + res_0 in one piece), and
// post into the skip convs (engine_pack.cpp pack_post4): every WN layer adds post . skip_j, 96 rows, into the first 96 rows
// of the skip sum -- s_0 = M_0 a_0 + c_0, s_j = (M_j a_j + c_j) + s_{j-1} -- and the chain launch has no post GEMM:
// x1 <- x1 - s_{nl-1}. The compositions ask chain4_frames, not chain_rs_front: PIPER_HIP_CHAIN_RS=0 only moves the last
// res/skip conv, one launch per coupling layer, and leaves pre and post composed. Post is composed on pre's route only (the
// knob changes nothing where gate4_kernel does not run).
std::vector<FlowLayerPlan> Engine::plan_flow(int B, int Fmax, double fsum) const {
  const bool chain = pol_.chain16(fsum, true, H_, C_ / 2), col4 = pol_.chain4_frames((long)B * Fmax);
  std::vector<FlowLayerPlan> plan(rcls_.size());
  for (size_t ri = 0; ri < rcls_.size(); ++ri) {
    const Rcl& r = rcls_[ri];
    FlowLayerPlan& p = plan[ri];
    p.chain = chain;
    p.rs_front = chain && r.front4_ok && pol_.chain_rs_front((long)B * Fmax);
    const bool compose = chain && r.front4_ok && col4 && r.compose_pre_ok && plan_conv(r.in[0], Fmax, EPI_GATE, stage_tiled_).form == CONV_GATE12;
    p.compose_pre = pol_.compose_pre() && compose;
    p.compose_post = pol_.compose_post() && compose && r.compose_post_ok;
    p.pre_launch = !(chain && ri > 0) && !p.compose_pre;
    p.pre_col4 = p.pre_launch && chain && r.pre4pad && H_ == 192 && col4;
    if (ri > 0) plan[ri - 1].chain_has_next_pre = !p.compose_pre;
    for (size_t i = 0; i < r.rs.size(); ++i) p.rs_col4.push_back(r.rs4[i] && col4 && H_ == 192 && r.rs[i].rows <= 2 * H_);
  }
  return plan;
}

void Engine::group_begin(bool tiled) {
  grouping_ = true;
  group_tiled_ = tiled;
  group_cfg_ = -1;
  group_.clear();
  group_flops_ = group_bytes_ = 0;
}
void Engine::group_end() {
  grouping_ = false;
  if (group_.empty()) return;
  if (group_tiled_) {
    group_tiled_ = false;
    // longest kernel first: workgroups are dispatched in grid order (z slowest)
    std::stable_sort(group_.begin(), group_.end(), [](const ConvP& a, const ConvP& b) { return a.ntaps > b.ntaps; });
    ConvG g{};
    int n = 0, rows = 0, xhalo = 0;
    for (const ConvP& c : group_) {
      g.c[n++] = c;
      rows = std::max(rows, c.rows);
      xhalo = std::max(xhalo, c.xhalo);
    }
    g.n = n;
    g.B = B_;
    const int cfg = group_cfg_, BM = CFG_BM[cfg], BN = CFG_BN[cfg];
    const int HALO = slab_halo(xhalo);
    const dim3 grid((group_ncols_ + BN - 1) / BN, (rows + BM - 1) / BM, n * B_);
    int kh = -1;
    if (prof_level_ >= 2) {
      char nm[96];
      snprintf(nm, sizeof(nm), "conv_mfma_group_kernel<%s,%d>", cfg == CFG_C ? "1,4,1,1,16" : "2,2,1,1,16", HALO);
      kh = kbegin(krow(std::string(nm)), group_flops_, group_bytes_);
    }
    launch::conv_tile_group(cfg, HALO, grid, tile_smem(2, BN, HALO), ls_, g);
    kend(kh);
    group_.clear();
    return;
  }
  // 4 waves per workgroup: 32 / 64 KB of slabs, so 4 / 2 workgroups share a CU and the <= 3 x ~420 workgroups of a
  // group run in one or two rounds (8 waves: 64 / 128 KB, five rounds, slower than one launch per conv). The convs that
  // need the 128-column slab go in a launch of their own: two resident workgroups per CU carry ~420 of them, not 1260.
  constexpr int NW = 4;
  // workgroups are dispatched in grid order (z slowest): the conv with the most taps goes first so that the longest
  // workgroups do not form the tail of the launch
  std::stable_sort(group_.begin(), group_.end(), [](const ConvP& a, const ConvP& b) { return a.ntaps > b.ntaps; });
  for (int wide = 0; wide < 2; ++wide) {
    ConvG g{};
    int n = 0, mt = 0;
    for (const ConvP& c : group_)
      if ((c.xhalo > 32) == (wide == 1)) {
        g.c[n++] = c;
        mt = std::max(mt, (c.rows + 31) / 32);
      }
    if (!n) continue;
    g.n = n;
    g.B = B_;
    const dim3 grid((group_ncols_ + 31) / 32, mt, n * B_);
    const double share = (double)n / (double)group_.size();
    const int kh = kbegin(prof_level_ >= 2 ? krow(wide ? "conv_splitk_group_kernel<4,2,128>" : "conv_splitk_group_kernel<4,2,64>") : 0,
                          group_flops_ * share, group_bytes_ * share);
    launch::conv_group(wide != 0, grid, splitk_smem(NW, 1, wide ? 128 : 64), ls_, g);
    kend(kh);
  }
  group_.clear();
}

bool Engine::can_group_sum() const {
  if (group_.size() < 2 || group_.size() > 3) return false;
  const ConvP& a = group_[0];
  for (const ConvP& c : group_)
    if (c.rows != a.rows || c.Cin != a.Cin || c.nchunks != a.nchunks || c.x_bs != a.x_bs || c.x_cs != a.x_cs ||
        c.r_bs != a.r_bs || c.r_cs != a.r_cs || c.in_slope != a.in_slope || c.epi != EPI_RESADD || c.xhalo > 96)
      return false;
  return true;
}
void Engine::group_end_sum(View out, const float* bias_sum, float alpha) {
  grouping_ = false;
  if (!can_group_sum()) throw std::runtime_error("internal: convs do not fit a K-concatenated launch");
  ConvP q = group_[0];
  q.nseg = (int)group_.size();
  for (int i = 0; i < q.nseg; ++i) {
    q.seg_x[i] = group_[i].x; q.seg_wp[i] = group_[i].wp;
    q.seg_ntaps[i] = group_[i].ntaps; q.seg_dil[i] = group_[i].dil; q.seg_padl[i] = group_[i].padl;
  }
  q.res2 = group_[1].res;
  q.res3 = q.nseg > 2 ? group_[2].res : nullptr;
  q.bias = bias_sum;
  q.out = out.p; q.o_bs = out.bs; q.o_cs = out.cs;
  q.epi = EPI_ACCUM; q.mode = 3; q.alpha = alpha;      // (acc + bias + residuals) * alpha, nothing read back
  q.tgroups = 1;
  const dim3 grid((group_ncols_ + 31) / 32, (q.rows + 31) / 32, B_);
  // (a 4-deep weight ring measured slower than 2: hifigan stage 0.345 vs 0.338 ms)
  // (a 16-deep ring -- a wave's whole K range in flight at entry, 256 registers, one workgroup per CU -- measured 59 us
  // against 30: profiles/r04_notes.md)
  const int kh = kbegin(prof_level_ >= 2 ? krow("conv_splitk_sum_kernel<4,2>") : 0, group_flops_, group_bytes_);
  launch::conv_group_sum(grid, splitk_smem(4, 1, 128), ls_, q);
  kend(kh);
  group_.clear();
}

// algorithmic FLOPs of a conv launch over `cols` valid columns: 2 * MACs per output column; algorithmic bytes: every input
// channel and every output row once per column, residual / read-modify-write operands once more each, the weights once
static void conv_cost(const PackedConv& pc, int epi, int mode, double cols, double& flops, double& bytes) {
  const bool rd_res = epi == EPI_RESADD || epi == EPI_ACCUM;
  const bool rd_old = epi == EPI_SUBFROM || epi == EPI_WNRS || (epi == EPI_ACCUM && (mode == 1 || mode == 2));
  const double out_rows = epi == EPI_GATE ? pc.split : pc.rows;
  flops = 2.0 * pc.macs_per_col * cols;
  bytes = 4.0 * (cols * (pc.Cin + out_rows * (1 + (rd_res ? 1 : 0) + (rd_old ? 1 : 0))) + (double)pc.rows * pc.Cin * pc.ntaps);
}

void Engine::conv(const PackedConv& pc, View x, View out, const int* lens, int len_mul, int Lmax, int epi, const ConvOpt& o) {
  if ((epi == EPI_GATE) != pc.gate) throw std::runtime_error("internal: gate epilogue/packing mismatch");
  ConvP p;
  p.x = x.p; p.x_bs = x.bs; p.x_cs = x.cs;
  p.wp = pc.wp; p.wp16 = pc.wp16; p.wpb = pc.wpb; p.wunscale = pc.wunscale; p.wpg4 = nullptr; p.bias = pc.bias;
  p.bias2 = o.bias2; p.bias2_bs = o.bias2_bs;
  p.out = out.p; p.o_bs = out.bs; p.o_cs = out.cs;
  p.res = o.res.p; p.r_bs = o.res.bs; p.r_cs = o.res.cs;
  p.out2 = o.out2.p; p.o2_bs = o.out2.bs; p.o2_cs = o.out2.cs;
  p.lens = lens; p.len_mul = len_mul;
  p.Cin = pc.Cin; p.rows = pc.rows; p.nchunks = pc.nchunks;
  p.ntaps = pc.ntaps; p.dil = pc.dil; p.padl = pc.padl; p.xhalo = (pc.ntaps - 1) * pc.dil;
  p.in_slope = o.in_slope; p.epi = epi; p.act = o.act; p.mode = o.mode; p.alpha = o.alpha;
  p.split = (epi == EPI_GATE) ? pc.split : (epi == EPI_WNRS ? (pc.rows > H_ ? H_ : 0) : 0);
  p.up = pc.up; p.padT = pc.padT; p.up_magic = pc.up ? (unsigned)((0x100000000ULL + pc.up - 1) / pc.up) : 0u;
  p.up_vec = 0; p.tpb = 1; p.tgroups = 1;      // (what a grouped launch runs with; a launch of its own takes the plan's)
  double kflops = 0, kbytes = 0;
  if (prof_level_ >= 2) {
    const std::vector<int32_t>& lh = (lens == d_tlens_) ? tlens_h_ : frames_h_;
    double cols = 0;
    for (int b = 0; b < B_; ++b) cols += (double)lh[b] * len_mul;      // valid columns over the batch
    conv_cost(pc, epi, o.mode, cols, kflops, kbytes);
  }
  const ConvPlan pl = plan_conv(pc, Lmax, epi, stage_tiled_);
  if (grouping_) {
    if (!(group_tiled_ ? pl.group_tiled : pl.group_splitk) || group_.size() >= 3 ||
        (!group_.empty() && (group_ncols_ != pl.ncols || (group_tiled_ && group_cfg_ != pl.group_cfg))))
      throw std::runtime_error(group_tiled_ ? "internal: conv does not fit a grouped tiled launch" : "internal: conv does not fit a grouped launch");
    group_cfg_ = pl.group_cfg;
    group_.push_back(p);
    group_ncols_ = pl.ncols;
    group_flops_ += kflops; group_bytes_ += kbytes;
    return;
  }
  p.up_vec = pl.up_vec; p.tpb = pl.tpb; p.tgroups = pl.tgroups;
  if (pl.form == CONV_GATE12) p.wpg4 = pc.wpg4;
  const int kh = prof_level_ >= 2 ? kbegin(krow(conv_row_name(pl, pc, matrix_sm_, pol_.prof_sites != 0, epi, len_mul)), kflops, kbytes) : -1;
  switch (pl.form) {
    case CONV_GATE12: launch::gate4(pl.grid, pl.smem, ls_, p); break;
    case CONV_SPLITK: launch::conv_splitk(pc.gate, pl.nw, pl.grid, pl.smem, ls_, p); break;
    case CONV_SPLITK16: launch::conv_splitk16(pc.gate, pl.grid, pl.smem, ls_, p, pl.half); break;
    case CONV_SPLIT: launch::conv_bf3(matrix_sm_, pl.cfg, pc.gate, pl.halo, pl.grid, pl.smem, ls_, p); break;
    case CONV_1X1: launch::conv1x1(pl.grid, ls_, p); break;
    case CONV_TILE: launch::conv_tile(pl.cfg, pc.gate, pl.halo, pl.grid, pl.smem, ls_, p); break;
  }
  kend(kh);
}

// The first WN gate conv of a coupling layer whose pre is composed into it (engine_pack.cpp pack_gate4pre): gate4_kernel's
// grid over the 96 channels of x0. The caller has asked plan_conv that the plain conv would take gate4_kernel here.
void Engine::gate_pre(const Rcl& r, View x0, View out, const int* lens, int Lmax, double cols, const float* b2) {
  const PackedConv& pc = r.in[0];
  ConvP p{};
  p.x = x0.p; p.x_bs = x0.bs; p.x_cs = x0.cs;
  p.wpg4 = r.gpre4; p.bias = r.gpre_bias;
  p.bias2 = b2; p.bias2_bs = cond_bs_;
  p.out = out.p; p.o_bs = out.bs; p.o_cs = out.cs;
  p.lens = lens; p.len_mul = 1;
  p.Cin = 96; p.rows = pc.rows; p.ntaps = pc.ntaps; p.dil = 1; p.padl = pc.padl; p.xhalo = pc.ntaps - 1;
  p.in_slope = 1.f; p.epi = EPI_GATE; p.split = pc.split;
  const double macs = (double)pc.rows * 96 * pc.ntaps;
  const int kh = kbegin(prof_level_ >= 2 ? krow("gate4pre_kernel") : 0, 2.0 * macs * cols, 4.0 * (cols * (96 + pc.split) + macs));
  launch::gate4pre(dim3((Lmax + 11) / 12, pc.split / 32, B_), ((size_t)16 * (96 + 4) + (size_t)6 * 64 * 12) * sizeof(float), ls_, p, r.gpre_tapb);
  kend(kh);
}

// mrf_kernel launch: the window geometry -- output columns per workgroup N = 16 * NCG * OU -- is chosen here. Few
// utterances: the launch is one or two rounds of workgroups over the 256 CUs, so the workgroup count should sit just under
// a multiple of 256 and a workgroup should be short; batches: many rounds, so large N (less halo recompute, fewer
// prologues) wins. Cost model: rounds x (MFMA columns of one workgroup incl. recompute + a fixed prologue / epilogue).
bool Engine::mrf_geo(const UpStage& st, int len_mul, bool tail, MrfGeo& best) const {
  const int CP = st.mrf_cp, NCG = CP == 32 ? 8 : 4, HU = CP == 32 ? 1 : 2;
  const int OUMAX = CP == 32 ? 4 : 3;      // 32 channels: 4 units per wave (N = 512) fill the 160 KB of LDS
  const int hx = st.mrf_hx, hxa = rup(hx, 16);
  auto geo = [&](int ou, MrfGeo& g) {
    g.ou = ou; g.N = 16 * NCG * ou;
    if (hxa + g.N + hx > mrf_ws(CP, ou)) return false;
    g.cu_lo = (hxa - hx) / 16; g.cu_hi = (hxa + g.N + hx + 15) / 16;
    g.nleft = hxa / 16 - g.cu_lo; g.nhalo = g.cu_hi - g.cu_lo - g.N / 16;
    return g.nhalo <= NCG * HU;
  };
  best = MrfGeo{};
  double best_cost = 0;
  MrfGeo forced;
  const int force = (pol_.mrf_ou >= 1 && pol_.mrf_ou <= OUMAX && geo((int)pol_.mrf_ou, forced)) ? (int)pol_.mrf_ou : 0;     // (tests / A-B; ignored when it does not fit)
  for (int ou = 1; ou <= OUMAX; ++ou) {
    MrfGeo g;
    if ((force && ou != force) || !geo(ou, g)) continue;
    double wgs = 0;
    const int stride = tail ? g.N - (POST_K - 1) : g.N;
    for (int b = 0; b < B_; ++b) wgs += (double)(((long)frames_h_[b] * len_mul + stride - 1) / stride);
    double work = 0, taps = 0;
    for (auto& P : st.mrf_ph) {
      const int lo = (hxa - P.e) / 16, hi = (hxa + g.N + P.e + 15) / 16;
      work += (double)(hi - lo) * 16 * P.ntaps;
      taps += P.ntaps;
    }
    double cost = std::ceil(wgs / 256.0) * (work + 16.0 * taps);      // prologue + epilogue ~ 16 columns' worth
    // 4 units per wave ran at the register limit (12 spilled VGPRs until the half-step B buffers of call 48): measured 3-5 % slower per column than 3 units at
    // batch (B=16: 1108 vs 1082 us, B=64: 4.29 vs 4.25 ms), but one round instead of two for a single utterance's last
    // stage (B=1: 84.6 vs 93.4 us) -- profiles/r03_notes.md
    if (ou == 4) cost *= 1.06;
    if (!best.ou || cost < best_cost) { best = g; best_cost = cost; }
  }
  return best.ou != 0;
}

void Engine::mrf(const UpStage& st, View x, View out, const int* lens, int len_mul, int Lmax, bool tail) {
  const int CP = st.mrf_cp, HU = CP == 32 ? 1 : 2;
  const int hx = st.mrf_hx, hxa = rup(hx, 16);
  MrfGeo best;
  if (!mrf_geo(st, len_mul, tail, best)) throw std::runtime_error("internal: no mrf_kernel geometry for this stage");
  MrfP p{};
  p.x = x.p; p.x_bs = x.bs; p.x_cs = x.cs;
  p.out = out.p; p.o_bs = out.bs; p.o_cs = out.cs;
  p.lens = lens; p.len_mul = len_mul;
  p.phases = static_cast<const MrfPhase*>(st.mrf_phases); p.nphases = (int)st.mrf_ph.size();
  p.wstream = st.mrf_w; p.wfloats = st.mrf_wfloats;
  p.C = st.ch; p.N = best.N; p.wcols = hxa + best.N + hx; p.hxa = hxa; p.cu_lo = best.cu_lo; p.cu_hi = best.cu_hi;
  p.nleft = best.nleft; p.nhalo = best.nhalo;
  p.slope = 0.1f;                            // modules.py LRELU_SLOPE
  p.alpha = 1.0f / (float)st.rb.size();
  p.stride = best.N; p.n0off = 0;
  p.post_w = nullptr; p.audio = nullptr; p.a_bs = 0; p.absmax = nullptr; p.post_slope = 0.01f;
  if (tail) {       // generator tail inside the stage kernel: windows overlap by the conv_post taps
    p.stride = best.N - (POST_K - 1); p.n0off = (POST_K - 1) / 2;
    p.post_w = post_w_; p.audio = audio_; p.a_bs = Ss_; p.absmax = absmax_;
  }
  double kflops = 0, kbytes = 0;
  if (prof_level_ >= 2) {
    double cols = 0;
    for (int b = 0; b < B_; ++b) cols += (double)frames_h_[b] * len_mul;
    double macs = 0;
    for (auto& cv : st.rb)
      for (auto& c : cv) macs += c.macs_per_col;
    kflops = 2.0 * macs * cols;
    kbytes = 8.0 * st.ch * cols + 4.0 * st.mrf_wfloats;      // one read of x, one write of the mean, the weights once
    if (tail) {
      kflops += 2.0 * cols * st.ch * POST_K;
      kbytes = 4.0 * (st.ch + 1) * cols + 4.0 * st.mrf_wfloats;   // one read of x, one write of the waveform
    }
  }
  dim3 grid((Lmax + p.stride - 1) / p.stride, B_);
  char nm[64];
  const bool split = matrix_bf3_ && pol_.mrf_split && st.mrf_wsplit != nullptr && matrix_sm_ < 2;
  if (split) {          // the same stage on the 16-bit pipe (kernels/mrf_split.h): same window geometry, the split weight stream
    p.wstream = st.mrf_wsplit; p.wfloats = st.mrf_wsplit_floats; p.wunscale = st.mrf_unscale;
    snprintf(nm, sizeof(nm), "mrf_split_kernel<%d,%d,%d,%d>", matrix_sm_, CP, best.ou, HU);
  } else {
    snprintf(nm, sizeof(nm), "mrf_kernel<%d,%d,%d>", CP, best.ou, HU);
  }
  const int kh = prof_level_ >= 2 ? kbegin(krow(std::string(nm)), kflops, kbytes) : -1;
  if (split) launch::mrf_split(matrix_sm_, CP, best.ou, grid, ls_, p);
  else launch::mrf(CP, best.ou, grid, ls_, p);
  kend(kh);
}

// LDS of attn_kernel / attn_long_kernel for utterances padded to T ids (kernels/attention.h: S | Vt | Qs | RK, RV | part)
size_t Engine::attn_smem(int T, bool global_scores) const {
  const int SP = rup(T, 64) + 1, VS = dk_ + 1 + (dk_ & 1);
  return ((global_scores ? 0 : (size_t)ATT_QB * SP) + (size_t)ATT_KCH * VS + (size_t)dk_ * ATT_QB +
          (size_t)2 * (2 * window_ + 1) * dk_ + 4 * ATT_QB * 16) * sizeof(float);
}
bool Engine::attn_scores_global(int T) const { return pol_.attn_long || attn_smem(T, false) > (size_t)160 * 1024; }

void Engine::layer_norm(View in, View out, const float* g, const float* b, int C, const int* lens, int Lmax) {
  LnP p;
  p.in = in.p; p.i_bs = in.bs; p.i_cs = in.cs;
  p.out = out.p; p.o_bs = out.bs; p.o_cs = out.cs;
  p.gamma = g; p.beta = b;
  p.lens = lens; p.C = C;
  if (C > LN_COLS * 32) throw std::runtime_error("LayerNorm over more than 256 channels is not supported");
  dim3 grid((Lmax + LN_COLS - 1) / LN_COLS, B_);
  const int kh = kbegin(prof_level_ >= 2 ? krow("ln_kernel") : 0, 0.0, 4.0 * 2.0 * C * (lens == d_tlens_ ? cols_ids_ : cols_frames_));
  launch::layer_norm(grid, stream_, p);
  kend(kh);
}

// DDSConv.forward (modules.py:117-129): one fused launch per layer (dds_layer16_kernel), ping-ponging between
// `out` and `tmp` so that the last layer lands in `out`; `in` must not alias the first layer's target.
void Engine::dds_params(const DdsW& d, View in, View out, View tmp, const DdsOpt* opt, std::vector<DdsP>& list) {
  int dil = 1;
  const int n = (int)d.c1x1.size();
  View cur = in;
  for (int i = 0; i < n; ++i) {
    const View dst = ((n - 1 - i) & 1) ? tmp : out;
    if (dst.p == cur.p) throw std::runtime_error("internal: DDSConv buffer aliasing");
    DdsP p{};
    if (opt && i == 0 && opt->pre_z) {
      p.pre_z = opt->pre_z; p.pre_z_bs = opt->pre_z_bs; p.pre_w = opt->pre_w; p.pre_b = opt->pre_b;
    }
    p.z_scale = opt ? opt->z_scale : nullptr;
    if (opt && i == n - 1 && opt->post_w16) {
      p.post_w16 = opt->post_w16; p.post_w4 = w4_of(opt->post_w16); p.post_bias = opt->post_bias; p.post_rows = opt->post_rows;
      p.post_out = opt->post_out.p; p.po_bs = opt->post_out.bs; p.po_cs = opt->post_out.cs;
      p.zin = opt->zin; p.zin_bs = opt->zin_bs; p.z_cs = opt->z_cs; p.c0 = opt->c0; p.c1 = opt->c1;
      p.zout = opt->zout; p.zout_bs = opt->zout_bs;
      p.inv_sqrt_h = 1.0f / std::sqrt((float)H_);
    }
    p.x = cur.p; p.x_bs = cur.bs; p.x_cs = cur.cs;
    p.out = dst.p; p.o_bs = dst.bs; p.o_cs = dst.cs;
    p.dw_w = d.dw_w[i]; p.dw_b = d.dw_b[i]; p.dw_k = ksz_; p.dw_dil = dil;
    p.g1 = d.g1[i]; p.b1 = d.b1[i]; p.g2 = d.g2[i]; p.b2 = d.b2[i];
    p.bias = d.c1x1[i].bias;
    p.wp16 = d.w16[i];
    p.wp4 = w4_of(d.w16[i]);
    p.nchunks = d.c1x1[i].nchunks;
    p.lens = d_tlens_; p.H = H_;
    list.push_back(p);
    dil *= ksz_;
    cur = dst;
  }
}

// algorithmic bytes of one DDSConv layer launch: x in, out (+ the fused 1x1 conv's rows), the 1x1 matrix (+ the fused one)
double Engine::dds_bytes(const DdsP& p) const {
  return 4.0 * (cols_ids_ * (2.0 * H_ + p.post_rows) + (double)H_ * H_ + (double)p.post_rows * H_);
}

void Engine::dds(const DdsW& d, View in, View out, View tmp, const DdsOpt* opt) {
  std::vector<DdsP> list;
  dds_params(d, in, out, tmp, opt, list);
  // Small calls of the 192-channel voices: 4-column workgroups on 4x the CUs (kernels/dds4.h). Every layer of the chain
  // needs its matrices in the 4x4x1 order; the form reads 4x the weight bytes, hence the column limit.
  bool four = H_ == 192 && ksz_ <= 3 && pol_.chain4((long)B_ * Tg_);
  for (const DdsP& p : list) four = four && p.wp4 && (!p.post_w16 || p.post_w4);
  for (const DdsP& p : list) {
    if (four) {
      const int kh4 = kbegin(prof_level_ >= 2 ? krow("dds_layer4_kernel") : 0, 0.0, dds_bytes(p));
      DdsP p4 = p;
      p4.xcd = xcd_period_;
      launch::dds_layer4(dim3((Tg_ + 3) / 4, B_), col4_smem(), stream_, p4);
      kend(kh4);
      continue;
    }
    const int kh = kbegin(prof_level_ >= 2 ? krow(p.nchunks == 3 ? "dds_layer16_kernel<3>" : p.nchunks == 6 ? "dds_layer16_kernel<6>"
                                                                                       : "dds_layer16_kernel<8>") : 0, 0.0, dds_bytes(p));
    const dim3 grid16((Tg_ + 15) / 16, B_);
    const size_t smem16 = ((size_t)2 * p.nchunks * 32 * 16 + 16 * 16 + 16 * 3 * 16) * sizeof(float);     // Y, Z, red, the spline tail's S
    // <3> / <6> are compiled for exactly 96 / 192 padded channels; <8> takes any width up to 256
    launch::dds_layer(p.nchunks, grid16, smem16, stream_, p);
    kend(kh);
  }
}

void Engine::set_profile(int level) {
  prof_level_ = level;
  prof_on_ = level > 0;
}
int Engine::krow(const char* name) {
  for (size_t i = 5; i < prof_.size(); ++i)
    if (!strcmp(prof_[i].name, name)) return (int)i;
  prof_.push_back(ProfileRow{name});
  return (int)prof_.size() - 1;
}
int Engine::krow(const std::string& name) {
  for (size_t i = 5; i < prof_.size(); ++i)
    if (name == prof_[i].name) return (int)i;
  names_.push_back(name);
  prof_.push_back(ProfileRow{names_.back().c_str()});
  return (int)prof_.size() - 1;
}
void Engine::lngemm(View y, const float* g, const float* b, View x, const float* w16, const float* bias, int rows,
                    View out, int T, double flops, const float* parts, int nparts, const float* pbias, const LnSecond* second) {
  // algorithmic bytes: y in, LN(y) out, the conv's rows out, the FFN's partial outputs in; weights once
  const double kbytes = 4.0 * (cols_ids_ * (2.0 * H_ + rows + (parts ? (double)nparts * H_ : 0.0)) + (double)rows * H_);
  LnGemmP p{};
  p.in = y.p; p.in_bs = y.bs; p.in_cs = y.cs;
  p.gamma = g; p.beta = b;
  p.xout = x.p; p.x_bs = x.bs; p.x_cs = x.cs;
  p.w16 = w16; p.bias = bias; p.rows = rows;
  p.out = out.p; p.o_bs = out.bs; p.o_cs = out.cs;
  p.lens = d_tlens_;
  // small calls: 4-column workgroups on the 4x4x1 MFMA (kernels/col4.h), like Engine::dds
  if (parts) {        // y = (View y: the residual) + pbias + the fused FFN's partial outputs (ffn_kernel)
    const int Tp = rup(T, 4);
    p.parts = parts; p.nparts = nparts; p.pbias = pbias;
    p.p_bs = (long)nparts * H_ * Tp;
    if (!(pol_.chain4((long)B_ * T) && w4_of(w16))) throw std::runtime_error("internal: FFN partials without the 4-column consumer");
  }
  if (second && !(pol_.chain4((long)B_ * T) && second->w4)) throw std::runtime_error("internal: stacked convs without the 4-column form");
  if (const float* w4 = pol_.chain4((long)B_ * T) ? (second ? second->w4 : w4_of(w16)) : nullptr) {
    p.w16 = w4;
    p.xcd = xcd_period_;
    if (kt_on_ && out.p == qkv_ && rows == 3 * H_) { p.kT = kT_; p.vQ = vQ_; p.kt_bs = (long)Ts_ * H_; kt_valid_ = true; }      // attn4_kernel follows
    if (second) {
      p.split = second->split; p.out2 = second->out2.p; p.o2_bs = second->out2.bs; p.o2_cs = second->out2.cs;
      p.bias2 = second->bias2; p.bias2_bs = second->bias2_bs;
    }
    const int kh4 = kbegin(prof_level_ >= 2 ? krow("lngemm4_kernel") : 0, flops, kbytes);
    launch::lngemm4(dim3((T + 3) / 4, B_, (rows + 191) / 192), col4_smem(), stream_, p);
    kend(kh4);
    return;
  }
  const int kh = kbegin(prof_level_ >= 2 ? krow("lngemm_kernel<6>") : 0, flops, kbytes);
  const size_t smem = ((size_t)192 * 16 + 16 * 16) * sizeof(float);
  launch::lngemm(dim3((T + 15) / 16, B_, (rows + 191) / 192), smem, stream_, p);
  kend(kh);
}

// A plain 1x1 conv over 192 input channels of a small call on 4-column workgroups (colchain4_kernel mode 3); false: the
// caller launches the conv kernel instead. `w16`: the conv's pack16 matrix (its pack4 twin is looked up).
bool Engine::conv1x1_col4(const float* w16, const float* bias, int rows, View in, View out, const int* lens, int B, int Lmax,
                          double flops, const float* bias2, long bias2_bs, const float* w4direct, int kin, long max_cols) {
  const bool small = pol_.chain4((long)B * Lmax, max_cols);
  const float* w4 = (H_ == 192 && small) ? (w4direct ? w4direct : w4_of(w16)) : nullptr;
  if (!w4) return false;
  ColP cp{};
  cp.in1 = in.p; cp.in1_bs = in.bs; cp.in1_cs = in.cs; cp.K1 = kin;
  cp.w1 = w4; cp.b1 = bias; cp.rows1 = rows;
  cp.mode = 3;
  cp.xcd = xcd_period_;
  cp.res = bias2; cp.res_bs = bias2_bs;
  cp.out = out.p; cp.out_bs = out.bs; cp.out_cs = out.cs;
  cp.lens = lens;
  if (kt_on_ && out.p == qkv_ && rows == 3 * H_) { cp.kT = kT_; cp.vQ = vQ_; cp.kt_bs = (long)Ts_ * H_; kt_valid_ = true; }      // attn4_kernel follows
  const double cols = lens == d_tlens_ ? cols_ids_ : cols_frames_;
  const int kh4 = kbegin(prof_level_ >= 2 ? krow("colchain4_kernel<false>") : 0, flops, 4.0 * (cols * (kin + rows) + (double)rows * kin));
  launch::colchain4(dim3((Lmax + 3) / 4, B, (rows + 191) / 192), col4_smem(), stream_, cp);
  kend(kh4);
  return true;
}

// conv_o + residual + norm_layers_1 of an encoder layer in one launch (mode 0: the 192 x 192 GEMM fits one workgroup per
// 16 columns, or per 4 on small calls); x is the residual and the output
void Engine::conv_o_ln(const EncLayer& e, View att, View x, int B, int T, double tsum) {
  ColP cp{};
  cp.in1 = att.p; cp.in1_bs = att.bs; cp.in1_cs = att.cs; cp.K1 = H_;
  cp.w1 = e.o16; cp.b1 = e.o.bias; cp.rows1 = H_; cp.mode = 0;
  cp.res = x.p; cp.res_bs = x.bs; cp.res_cs = x.cs;
  cp.gamma = e.g1; cp.beta = e.b1;
  cp.out = x.p; cp.out_bs = x.bs; cp.out_cs = x.cs;
  cp.lens = d_tlens_;
  colchain(cp, B, T, 2.0 * tsum * e.o.macs_per_col);
}

// Small calls: the res/skip 1x1 conv of WN layer `layer` on 4-column workgroups (colchain4_kernel mode 2), one part per 192
// rows: fh += res rows, fskip (+)= skip rows. Post composed: the skip rows are post . skip_i, 96 of them. Pre composed, first
// layer: the res part also adds pre(x0) -- fh is written as the whole hidden state, not read.
void Engine::wn_res_skip4(const Rcl& r, int layer, const FlowLayerPlan& pl, View x0, View facts, View fh, View fskip, int B, int Fmax, double fsum) {
  const int half = C_ / 2;
  ColP cp{};
  cp.in1 = facts.p; cp.in1_bs = facts.bs; cp.in1_cs = facts.cs; cp.K1 = H_;
  cp.w1 = r.rs4[layer]; cp.b1 = r.rs[layer].bias; cp.rows1 = r.rs[layer].rows;
  if (pl.compose_post) { cp.w1 = r.rsp4[layer]; cp.b1 = r.rsp_bias[layer]; cp.rows1 = r.rs[layer].rows - H_ + half; }
  cp.mode = 2; cp.first = layer == 0 ? 1 : 0;
  cp.xcd = xcd_period_;
  cp.x1 = fh.p; cp.x1_bs = fh.bs; cp.x1_cs = fh.cs;
  cp.out = fskip.p; cp.out_bs = fskip.bs; cp.out_cs = fskip.cs;
  cp.lens = lens_b_;
  const bool hpre = pl.compose_pre && layer == 0;
  if (hpre) { cp.in0 = x0.p; cp.in0_bs = x0.bs; cp.in0_cs = x0.cs; cp.w2 = w4_of(r.pre16); cp.b2 = r.pre.bias; cp.rows2 = H_; }
  const int kh4 = kbegin(prof_level_ >= 2 ? krow("colchain4_kernel<false>") : 0,
                         2.0 * fsum * ((double)cp.rows1 * H_ + (hpre ? r.pre.macs_per_col : 0)),
                         4.0 * (fsum * (H_ + 2.0 * cp.rows1) + (double)cp.rows1 * H_ + (hpre ? half * (fsum + H_) : 0)));
  launch::colchain4(dim3((Fmax + 3) / 4, B, (cp.rows1 + 191) / 192), col4_smem(hpre), stream_, cp);
  kend(kh4);
}

// post + "x1 -= m" + the next coupling layer's pre over the updated half, one launch (mode 1). rs_front: the last WN layer's
// res/skip conv (skip rows only) runs in front, from facts. Post composed: the skip sum is m -- no post GEMM, K1 = half and
// a null w1 tell the kernel so. Pre of the next layer composed: its gate conv reads x0 itself, no second GEMM here.
void Engine::coupling_chain(const Rcl& r, const Rcl* next, const FlowLayerPlan& pl, View x1, View facts, View fskip, View fh, int B, int Fmax, double fsum) {
  const int half = C_ / 2, nl = (int)r.in.size();
  ColP cp{};
  cp.in1 = fskip.p; cp.in1_bs = fskip.bs; cp.in1_cs = fskip.cs; cp.K1 = H_;
  cp.w1 = r.post16; cp.b1 = r.post.bias; cp.rows1 = half; cp.mode = 1;
  cp.x1 = x1.p; cp.x1_bs = x1.bs; cp.x1_cs = x1.cs;
  if (pl.chain_has_next_pre) {
    if (next->in_off != r.out_off) throw std::runtime_error("coupling layers do not alternate halves");
    cp.w2 = next->pre16; cp.b2 = next->pre.bias; cp.rows2 = H_;
    cp.out2 = fh.p; cp.o2_bs = fh.bs; cp.o2_cs = fh.cs;
  }
  cp.lens = lens_b_;
  if (pl.rs_front) {
    cp.in0 = facts.p; cp.in0_bs = facts.bs; cp.in0_cs = facts.cs;
    cp.w0 = r.rs4[nl - 1]; cp.b0 = r.rs[nl - 1].bias; cp.first = nl == 1 ? 1 : 0;
  }
  if (pl.compose_post) { cp.K1 = half; cp.w1 = nullptr; cp.b1 = nullptr; }
  if (pl.compose_post && pl.rs_front) { cp.w0 = r.rsp4[nl - 1]; cp.b0 = r.rsp_bias[nl - 1]; }
  colchain(cp, B, Fmax, 2.0 * fsum * ((pl.compose_post ? 0 : r.post.macs_per_col) + (cp.w2 ? next->pre.macs_per_col : 0) +
                                      (pl.rs_front ? (pl.compose_post ? (double)half * H_ : r.rs[nl - 1].macs_per_col) : 0)));
}

// Whether a chain launch takes its 4-column form (colchain4_kernel), per mode. Mode 0 runs on ids, mode 1 on frames: separate
// column limits (profiles/r03_notes.md). Mode 1 without w1: post composed into the skip convs, in1 (96 rows) is m as it is.
static bool conv_o_ln_col4(const LaunchPolicy& pol, const ColP& p, long cols) { return pol.chain4(cols) && p.w1 && p.K1 == 192 && p.rows1 == 192; }
static bool coupling_chain_col4(const LaunchPolicy& pol, const ColP& p, long cols) { return pol.chain4_frames(cols) && p.K1 == (p.w1 ? 192 : 96) && p.rows1 == 96 && (!p.w2 || p.rows2 <= 192); }

// Modes 0 and 1: 4 columns per workgroup on small calls whose matrices have their pack4 twins, else 16 (colchain_kernel).
void Engine::colchain(const ColP& p, int B, int Lmax, double flops) {
  // algorithmic bytes: GEMM input, the residual / x1 read and written, the second GEMM's output; weights once
  const double cols = p.lens == d_tlens_ ? cols_ids_ : cols_frames_;
  const double kbytes = 4.0 * (cols * (p.K1 + 2.0 * p.rows1 + (p.w2 ? p.rows2 : 0)) + (p.w1 ? (double)p.rows1 * p.K1 : 0.0) +
                               (p.w2 ? (double)p.rows2 * p.rows1 : 0.0));
  if (p.mode == 0 ? conv_o_ln_col4(pol_, p, (long)B * Lmax) : coupling_chain_col4(pol_, p, (long)B * Lmax)) {
    const float* w1 = p.w1 ? w4_of(p.w1) : nullptr;
    const float* w2 = p.w2 ? w4_of(p.w2) : nullptr;
    if ((w1 || !p.w1) && (!p.w2 || w2)) {
      ColP q = p;
      q.w1 = w1; q.w2 = w2;
      q.xcd = xcd_period_;
      const double kb0 = q.w0 ? 4.0 * (cols * 192.0 + (q.w1 ? 192.0 : 96.0) * 192.0) : 0.0;      // the front conv: its input, its weights
      const int kh4 = kbegin(prof_level_ >= 2 ? krow(q.w0 ? "colchain4_kernel<true>" : "colchain4_kernel<false>") : 0, flops, kbytes + kb0);
      launch::colchain4(dim3((Lmax + 3) / 4, B), col4_smem(), stream_, q);
      kend(kh4);
      return;
    }
  }
  if (p.w0 || !p.w1) throw std::runtime_error("internal: a res/skip conv in front of a chain that does not take the 4-column form");
  const int kh = kbegin(prof_level_ >= 2 ? krow("colchain_kernel<6>") : 0, flops, kbytes);
  const size_t smem = ((size_t)2 * 6 * 32 * 16 + 16 * 16) * sizeof(float);
  launch::colchain(dim3((Lmax + 15) / 16, B), smem, stream_, p);
  kend(kh);
}

int Engine::kbegin(int row, double flops, double bytes) {
  if (prof_level_ < 2) return -1;
  hipEvent_t a, b;
  if (ev_pool_.size() >= 2) {
    a = ev_pool_.back(); ev_pool_.pop_back();
    b = ev_pool_.back(); ev_pool_.pop_back();
  } else {
    PE_HIP(hipEventCreate(&a));
    PE_HIP(hipEventCreate(&b));
  }
  PE_HIP(hipEventRecord(a, ls_));
  kev_.push_back(KEvent{row, flops, bytes, a, b});
  return (int)kev_.size() - 1;
}
void Engine::kend(int h) {
  if (h >= 0) PE_HIP(hipEventRecord(kev_[h].b, ls_));
}
const std::vector<ProfileRow>& Engine::profile() {
  if (!kev_.empty()) {
    PE_HIP(hipStreamSynchronize(stream_));
    for (auto& k : kev_) {
      float ms = 0;
      PE_HIP(hipEventElapsedTime(&ms, k.a, k.b));
      prof_[k.row].ms += ms;
      prof_[k.row].flops += k.flops;
      prof_[k.row].bytes += k.bytes;
      prof_[k.row].launches += 1;
      ev_pool_.push_back(k.a);
      ev_pool_.push_back(k.b);
    }
    kev_.clear();
  }
  return prof_;
}
void Engine::reset_profile() {
  profile();
  for (auto& r : prof_) { r.ms = 0; r.flops = 0; r.launches = 0; r.bytes = 0; }
}
void Engine::prof_begin() {
  if (prof_on_) PE_HIP(hipEventRecord(ev0_, stream_));
}
void Engine::prof_end(int row, double flops) {
  if (!prof_on_) return;
  PE_HIP(hipEventRecord(ev1_, stream_));
  PE_HIP(hipEventSynchronize(ev1_));
  float ms = 0;
  PE_HIP(hipEventElapsedTime(&ms, ev0_, ev1_));
  prof_[row].ms += ms;
  prof_[row].flops += flops;
  prof_[row].launches += 1;
}

}  // namespace pe
