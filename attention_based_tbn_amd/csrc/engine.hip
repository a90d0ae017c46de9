// BN-Inception backbone engine: the whole per-modality conv stack as one natively scheduled
// program of HIP launches on one stream (forward train / forward eval / backward).
//
// Graph: reference core/models/bn_inception_audio.py:58-404 (layers) and :437-1003 (dataflow, concat
// order 1x1 | 3x3 | double-3x3 | pool) with the 7x7 stem of core/models/bn_inception.py:75-77.
// MI355X-first choices (vs. the reference's one nn.Module call per layer):
//   * NHWC activations; every branch writes straight into its channel slice of the block's
//     concat buffer (no torch.cat copies);
//   * the 1x1 convs that read the same block input -- 1x1, 3x3_reduce, double_3x3_reduce AND pool_proj (a 3x3
//     average pool and a bias-free 1x1 conv commute exactly, so the pool runs on pool_proj's few OUTPUT channels) --
//     run as ONE GEMM forward, one weight-gradient GEMM and one data-gradient GEMM (their parameters are adjacent
//     in the flat parameter arrays): the block input's gradient is written once instead of accumulated;
//   * training-mode BatchNorm statistics are produced by the conv epilogue (no extra pass over y), and the
//     BN-BACKWARD reduction (sum g, sum g*xhat) by the epilogue of the data-gradient GEMM that finishes dz
//     (no extra pass over dz and y either);
//   * the BN steps of the independent layers of a block run as batched (multi-tensor) launches;
//   * all parameters of a backbone live in 6 flat arrays, gradients likewise -> the data-parallel
//     all-reduce and the optimizer touch a handful of large tensors (RCCL/xGMI friendly);
//   * the caller owns all memory: one workspace blob sized by tbn_backbone_workspace_bytes().
#include <string>
#include <vector>
#include <cstring>
#include <cstdio>

#include <cstdlib>
#include "tbn_common.h"
#include "tbn_kernels.h"
#include "../../include/tbn_hip.h"

namespace {

struct BlockSpec {
  const char* name;
  int cin, c1, c3r, c3, cdr, cd1, cd2;
  int pool;  // 0 avg->proj, 1 max(s1)->proj, 2 max(s2) pass-through
  int cp, stride;
};
const BlockSpec kBlocks[] = {
    {"3a", 192, 64, 64, 64, 64, 96, 96, 0, 32, 1},     {"3b", 256, 64, 64, 96, 64, 96, 96, 0, 64, 1},
    {"3c", 320, 0, 128, 160, 64, 96, 96, 2, 0, 2},     {"4a", 576, 224, 64, 96, 96, 128, 128, 0, 128, 1},
    {"4b", 576, 192, 96, 128, 96, 128, 128, 0, 128, 1}, {"4c", 576, 160, 128, 160, 128, 160, 160, 0, 128, 1},
    {"4d", 608, 96, 128, 192, 160, 192, 192, 0, 128, 1}, {"4e", 608, 0, 128, 192, 192, 256, 256, 2, 0, 2},
    {"5a", 1056, 352, 192, 320, 160, 224, 224, 0, 128, 1}, {"5b", 1024, 352, 192, 320, 192, 224, 224, 1, 128, 1},
};
const int kNumBlocks = 10;
// gradient buckets of a backward pass (tbn_backbone_grads.bucket_cb): [5a, 5b] and [4a .. 4e] as they become final, the rest
// (stem, 3a .. 3c) when the pass returns.  Parameter share of the 10.24 M weights: 43.8 % / 46.6 % / 9.6 %.
const int kGradBuckets = 2;
const int kBucketBlock[kGradBuckets] = {8, 3};
const int kMaxParts = TBN_CONV_MAXSEG;

struct Buf {
  int H, W, C;
  size_t off, doff;  // float offsets of z and dz in the workspace
};

// one reference conv + BatchNorm + ReLU: a column range ("part") of a GEMM
struct Part {
  std::string name;
  int cout, col0;
  int dst_buf, dst_choff;   // where z = relu(bn(.)) goes (a channel slice of a concat buffer)
  size_t c_off;             // offset in the flat per-channel arrays
  bool pooled = false;      // BN input = avg_pool3x3(conv output columns): pool_proj riding in the fused 1x1 GEMM
  size_t y2_off = 0;        // pooled: the pooled conv output = BN input (P x cout, pitch cout)
  size_t yraw_off = 0;      // pooled, eval mode: raw conv output (P x cout, pitch cout)
  size_t bpart_off = 0;     // BN-backward partials written by the data-gradient epilogue of conv `red_src`
  int red_src = -1;         // -1: own reduce kernel
  int slot = 0;             // pooled: scratch slot of its forward statistics partials
  int slot_b = 0;           // the same in branch mode (side-stream work keeps to slots 2 and 3)
};

struct Conv {   // one GEMM: up to four parts that read the same input (adjacent in the flat parameter arrays)
  int nparts;
  Part parts[kMaxParts];
  int cin, cout, k, stride, pad;
  int inbuf, inH, inW, outH, outW;
  size_t w_off, c_off;
  size_t y_off;                 // training: raw conv output (P x cout); becomes dy in place during backward
  int slot = 0;                 // forward statistics scratch slot
  int slot_b = 0;               // the same in branch mode (see tbn_backbone_plan::ops_b)
  // forward launch choices, PER MODE ([0] eval epilogue, [1] training epilogue): the two modes are tuned separately and a
  // validation pass at the training shape must not overwrite what training was tuned to (round-2 advisor finding)
  struct FwdTune {
    int mt = 1, nt = 1, stages = 0;   // tile / LDS stages (0 = default)
    int halo = 0;                     // kernel variant: 1 LDS-halo, 2 LDS-DMA, 3 split-K tile
    bool pair = false;                // sibling pair in one launch (first member holds the decision)
    int p_variant = 1, p_mt = 1, p_nt = 1;
    float t = 0.f;                    // autotune: best single-launch time (ms)
  } ft[2];
  int d_mt = 1, d_nt = 1, d_stages = 0; // dgrad tile
  int d_halo = 0;               // kernel variant of the data-gradient GEMM
  // sibling pairing (3x3 | double_3x3_1 of a block: independent GEMMs issued as ONE launch, tbn_launch_conv_pair)
  int pair_next = -1, pair_prev = -1;     // the first member points at the second and vice versa
  bool pair_dgrad = false;                // decided by the autotuner (first member holds the decision)
  int pd_variant = 1, pd_mt = 1, pd_nt = 1;
  float t_dgrad = 0.f;                    // autotune: best single-launch time (ms)
  int w_mt = 0, w_nt = 0;       // wgrad tile (0 = heuristic)
  bool stem;
  bool dgrad_accum;    // dgrad adds into d(inbuf)
  bool need_dgrad;
  int fuse_pool = -1;  // training: index of the max pool that is the ONLY consumer of this conv's BN-ReLU output
  // BN layers whose dz this conv's data gradient finishes (it is the last writer of d(inbuf)): their BN-backward
  // reduce runs in its epilogue.  Ascending column order of inbuf.
  int nred = 0;
  int red_conv[kMaxParts], red_part[kMaxParts];
};

struct Pool {
  int kind;  // 0 avg3, 1 max
  int inbuf, outbuf, out_choff, stride, pad;
  size_t argmax_off;   // bytes
  bool bwd_accum;
  bool fused = false;  // training: executed inside its producer conv's BN apply / BN backward (see Conv::fuse_pool)
};

struct BnStep {   // BN (+ReLU) of up to four independent layers: one finalize + one apply launch (three in backward)
  int n;
  int conv[kMaxParts], part[kMaxParts];
  int slot0 = 0;  // first BN-backward scratch slot (partials, coefficients) of its members: 2 for side-stream steps
};

// OP_FORK / OP_JOIN only occur in the branch-mode program (ops_b): forward, FORK makes the side stream wait for the
// launch stream and JOIN the launch stream for the side stream; the backward pass walks the list in reverse with the
// two exchanged
enum { OP_CONV = 0, OP_POOL = 1, OP_BN = 2, OP_PREPOOL = 3, OP_FORK = 4, OP_JOIN = 5 };
struct Op {
  int kind;
  int idx;   // conv / pool / bn-step index; OP_PREPOOL: conv index
  int part;  // OP_PREPOOL: part index
  int side;  // branch mode: 1 = runs on the side stream
};

int pool_out(int in, int k, int stride, int pad, bool ceil_mode) {
  int num = in + 2 * pad - k;
  int o = (ceil_mode ? (num + stride - 1) / stride : num / stride) + 1;
  if (ceil_mode && (o - 1) * stride >= in + pad) --o;
  return o;
}

}  // namespace

struct tbn_backbone_plan {
  int cin0, frames, H, W;
  // (the fields below are filled from stem_geom, tbn_kernels.h: the one statement of these numbers)
  // stem conv as executed: 4 rows / stride 1 of the zero-bordered 2x2 space-to-depth image (stem_H, stem_W, cp = 4*cin0),
  // a filter row = kw = 4 pixels * cp contiguous floats, K = 4 * kw packed (pool.hip, conv_igemm.hip ROWMODE)
  int cp, kw;
  int stem_rows, stem_stride, stem_pad, stem_H, stem_W;
  // stem_mode 1 ("row runs", many input channels): 7 rows / stride 2 of a zero-bordered NHWC image instead (cp = cin0,
  // kw = 7*cin0 rounded up to x4); stem_K = multiplied K columns of the forward GEMM (rows * kw rounded up to x32)
  int stem_mode, stem_K;
  std::vector<Buf> bufs;
  std::vector<Conv> convs;
  std::vector<Pool> pools;
  std::vector<BnStep> bns;
  std::vector<Op> ops;
  // Branch mode (a side stream is given and nothing is capturing): the same layers as `ops`, ordered and tagged so that
  // the two independent chains of an inception block run on two streams --
  //   launch stream: 1x1 group -> BN -> double_3x3_1 -> BN -> double_3x3_2 -> BN
  //   side stream  : [pool of the block input] -> 3x3 -> [pool_proj] -> BN(3x3, pool_proj)
  // forked once the 1x1 group's BN is done, joined at the end of the block (reference dataflow
  // core/models/bn_inception_audio.py:437-1003: the four branches only meet at the concat, :485-493).  One chain's BN /
  // pool passes and 6-us finalize bubbles then sit under the other chain's GEMMs.  Sibling-pair launches (which put
  // 3x3 and double_3x3_1 into ONE grid) are not used in this mode.
  std::vector<Op> ops_b;
  // Riders (tbn_backbone_params.flags & TBN_BACKBONE_RIDERS, one-chain program, training): per inception block the BN
  // members whose elementwise pass runs inside the grid of a sibling GEMM launch (tbn_kernels.h RiderP)
  struct BlockRiders {
    int bn_g, bn_mid, bn_d2;        // the block's BN steps: fused 1x1 group | 3x3, double_3x3_1, pool_proj | double_3x3_2
    int c3, cd2;                    // hosts: forward apply of the 1x1 range rides on c3's launch (or its pair launch); forward
                                    // apply of 3x3 / pool_proj and all backward riders on double_3x3_2's forward / data gradient
    unsigned g_defer, mid_defer;    // member bit masks of bn_g / bn_mid that ride
  };
  std::vector<BlockRiders> riders;
  std::vector<int> bn_block;        // BN step -> block index (-1: stem)
  // first conv / first op (one-chain program, branch program) of every inception block: a backward walk that has finished
  // op block_op[b] has issued the weight gradient of every conv from block_conv[b] on -- a SUFFIX of the flat weight
  // tensor (convs are laid out in plan order), which is what tbn_backbone_grads.bucket_cb hands to the caller
  int block_conv[10], block_op[10], block_op_b[10];
  int rider_launches[2] = {0, 0};   // conv launches of the last forward / backward pass that carried a rider (diagnostics)
  int out_buf;
  size_t weight_floats, chan_floats;
  // workspace layout (float offsets unless noted)
  size_t x0_off, stats_off, partial_off, coef_off, wsplit_off, wt_off, wpack_off, dwpack_off;
  size_t diag_fold_off;   // -DTBN_DIAG=1 builds: ones | zeros (2 x 2048 floats) for the operand-staging cost probe (TBN_DIAG_FOLD=1)
  FlipTab flip;  // data-gradient weights: one flip/transpose launch per backward pass
  size_t partial_floats, wsplit_floats, wt_floats;
  size_t argmax_bytes_off, total_bytes_train, total_bytes_eval;
  size_t eval_floats;
  // fork/join events for the optional aux (weight-gradient) stream; created on first use.  One event per fork (a
  // backward pass never records an event twice: re-recording inside a stream capture is where ROCm 7.2 fell over)
  // + one for the join.
  static const int kEvents = 128;
  hipEvent_t ev[kEvents];
  int n_ev = 0;
};

namespace {

int add_buf(tbn_backbone_plan* P, int H, int W, int C) {
  Buf b;
  b.H = H;
  b.W = W;
  b.C = C;
  b.off = b.doff = 0;
  P->bufs.push_back(b);
  return (int)P->bufs.size() - 1;
}

int add_conv(tbn_backbone_plan* P, int nparts, const std::string* names, const int* couts, int cin, int k, int stride,
             int pad, int inbuf, const int* dst_buf, const int* dst_choff, bool stem) {
  Conv c;
  c.nparts = nparts;
  c.cout = 0;
  c.c_off = P->chan_floats;
  for (int i = 0; i < nparts; ++i) {
    Part& q = c.parts[i];
    q.name = names[i];
    q.cout = couts[i];
    q.col0 = c.cout;
    q.dst_buf = dst_buf[i];
    q.dst_choff = dst_choff[i];
    q.c_off = c.c_off + c.cout;
    c.cout += couts[i];
  }
  c.cin = cin;
  c.k = k;
  c.stride = stride;
  c.pad = pad;
  c.inbuf = inbuf;
  c.inH = P->bufs[inbuf].H;
  c.inW = P->bufs[inbuf].W;
  c.outH = (c.inH + 2 * pad - k) / stride + 1;
  c.outW = (c.inW + 2 * pad - k) / stride + 1;
  c.stem = stem;
  c.w_off = P->weight_floats;
  P->weight_floats += (size_t)c.cout * k * k * cin;
  P->chan_floats += c.cout;
  c.need_dgrad = !stem;
  c.dgrad_accum = false;
  c.y_off = 0;
  P->convs.push_back(c);
  Op o = {OP_CONV, (int)P->convs.size() - 1, 0, 0};
  P->ops.push_back(o);
  return o.idx;
}

int add_pool(tbn_backbone_plan* P, int kind, int inbuf, int outbuf, int out_choff, int stride, int pad) {
  Pool p;
  p.kind = kind;
  p.inbuf = inbuf;
  p.outbuf = outbuf;
  p.out_choff = out_choff;
  p.stride = stride;
  p.pad = pad;
  p.argmax_off = 0;
  p.bwd_accum = false;
  P->pools.push_back(p);
  Op o = {OP_POOL, (int)P->pools.size() - 1, 0, 0};
  P->ops.push_back(o);
  return o.idx;
}

// a BN step that only the branch-mode program uses (not appended to `ops`)
int add_bn_only(tbn_backbone_plan* P, int n, const int* conv, const int* part, int slot0) {
  BnStep s;
  s.n = n;
  s.slot0 = slot0;
  for (int i = 0; i < n; ++i) {
    s.conv[i] = conv[i];
    s.part[i] = part[i];
  }
  P->bns.push_back(s);
  return (int)P->bns.size() - 1;
}

int add_bn(tbn_backbone_plan* P, int n, const int* conv, const int* part) {
  const int bi = add_bn_only(P, n, conv, part, 0);
  Op o = {OP_BN, bi, 0, 0};
  P->ops.push_back(o);
  return bi;
}

// BN step over every (non-pooled) part of one conv
int add_bn_conv(tbn_backbone_plan* P, int ci) {
  int cs[kMaxParts], ps[kMaxParts], n = 0;
  for (int i = 0; i < P->convs[ci].nparts; ++i)
    if (!P->convs[ci].parts[i].pooled) {
      cs[n] = ci;
      ps[n++] = i;
    }
  return add_bn(P, n, cs, ps);
}

// rows of the GEMM's M dimension per workgroup tile = rows per statistics / reduce partial row: the split-K tile kernel
// (variant 3, layers of at most kSk4MaxRows rows) has 32-row wave tiles, every other kernel 128
constexpr int kSk4MaxRows = 32768;
inline int tile_rows(int variant, int mt) { return (variant == 3 ? 32 : 128) * mt; }

// false: the input size makes the reference graph itself inconsistent (its torch.cat of a stride-2 conv branch and the
// ceil-mode pass-through max pool raises)
bool build_graph(tbn_backbone_plan* P) {
  const int cin0 = P->cin0;
  {
    // the stem as executed: stem_geom (tbn_kernels.h) states the two layouts and the rule that picks one
    static const int use_rows = tbn_env_int("TBN_STEM_ROWS", 1, 0, 1);   // A/B runs: 0 = always s2d
    const StemGeom sg = stem_geom(cin0, P->H, P->W, use_rows ? STEM_LAYOUT_RULE : STEM_LAYOUT_S2D);
    P->cp = sg.cp;
    P->kw = sg.kw;
    P->stem_rows = sg.rows;
    P->stem_stride = sg.stride;
    P->stem_pad = sg.pad;
    P->stem_H = sg.H;
    P->stem_W = sg.W;
    P->stem_mode = sg.mode;
    P->stem_K = sg.K;
  }
  P->weight_floats = P->chan_floats = 0;
  const int x0 = add_buf(P, P->H, P->W, cin0);   // logical extent (the stored image is the bordered s2d form: plan_memory)
  // stem
  int h1 = (P->H + 6 - 7) / 2 + 1, w1 = (P->W + 6 - 7) / 2 + 1;
  const int c1 = add_buf(P, h1, w1, 64);
  {
    std::string n = "conv1_7x7_s2";
    int co = 64, db = c1, dc = 0;
    add_bn_conv(P, add_conv(P, 1, &n, &co, cin0, 7, 2, 3, x0, &db, &dc, true));
  }
  int hp = pool_out(h1, 3, 2, 0, true), wp = pool_out(w1, 3, 2, 0, true);
  const int p1 = add_buf(P, hp, wp, 64);
  add_pool(P, 1, c1, p1, 0, 2, 0);
  const int c2r = add_buf(P, hp, wp, 64);
  {
    std::string n = "conv2_3x3_reduce";
    int co = 64, db = c2r, dc = 0;
    add_bn_conv(P, add_conv(P, 1, &n, &co, 64, 1, 1, 0, p1, &db, &dc, false));
  }
  const int c2 = add_buf(P, hp, wp, 192);
  {
    std::string n = "conv2_3x3";
    int co = 192, db = c2, dc = 0;
    add_bn_conv(P, add_conv(P, 1, &n, &co, 64, 3, 1, 1, c2r, &db, &dc, false));
  }
  int h = pool_out(hp, 3, 2, 0, true), w = pool_out(wp, 3, 2, 0, true);
  int x = add_buf(P, h, w, 192);
  add_pool(P, 1, c2, x, 0, 2, 0);

  P->ops_b = P->ops;   // the stem is one chain: same program in both modes
  for (int bi = 0; bi < kNumBlocks; ++bi) {
    const BlockSpec& B = kBlocks[bi];
    const std::string pre = std::string("inception_") + B.name;
    P->block_conv[bi] = (int)P->convs.size();
    P->block_op[bi] = (int)P->ops.size();
    P->block_op_b[bi] = (int)P->ops_b.size();
    int oh = h, ow = w;
    if (B.stride == 2) {
      oh = (h + 2 - 3) / 2 + 1;
      ow = (w + 2 - 3) / 2 + 1;
    }
    const int ctot = B.c1 + B.c3 + B.cd2 + (B.pool == 2 ? B.cin : B.cp);
    const int O = add_buf(P, oh, ow, ctot);
    const int T1 = add_buf(P, h, w, B.c3r);
    const int T2 = add_buf(P, h, w, B.cdr);
    const int T3 = add_buf(P, h, w, B.cd1);
    // fused 1x1 group on the block input: 1x1 | 3x3_reduce | double_3x3_reduce | pool_proj.
    // reference: pool_proj(avg_pool3x3(x)).  A 3x3 / stride 1 / count_include_pad average and a (bias-free) 1x1
    // conv commute exactly, so the conv runs on the block input -- as a fourth column range of this GEMM -- and the
    // POOLING runs on its 32..128 output channels instead of the 192..1056 input channels.  The bias is added after
    // the pool (it is folded into the BN statistics / shift like everywhere else), where the reference adds it.
    int g, g_pp = -1, bn_g = -1;
    int c3 = -1, cd1 = -1, cd2 = -1, cpp = -1, pool_idx = -1, bn_d2 = -1;   // what the branch-mode program refers to
    {
      std::string names[kMaxParts];
      int couts[kMaxParts], db[kMaxParts], dc[kMaxParts], n = 0;
      if (B.c1) {
        names[n] = pre + "_1x1";
        couts[n] = B.c1;
        db[n] = O;
        dc[n] = 0;
        ++n;
      }
      names[n] = pre + "_3x3_reduce";
      couts[n] = B.c3r;
      db[n] = T1;
      dc[n] = 0;
      ++n;
      names[n] = pre + "_double_3x3_reduce";
      couts[n] = B.cdr;
      db[n] = T2;
      dc[n] = 0;
      ++n;
      if (B.pool == 0) {
        names[n] = pre + "_pool_proj";
        couts[n] = B.cp;
        db[n] = O;
        dc[n] = B.c1 + B.c3 + B.cd2;
        g_pp = n++;
      }
      g = add_conv(P, n, names, couts, B.cin, 1, 1, 0, x, db, dc, false);
      if (g_pp >= 0) P->convs[g].parts[g_pp].pooled = true;
      bn_g = add_bn_conv(P, g);
      if (g_pp >= 0) {
        Op o = {OP_PREPOOL, g, g_pp, 0};
        P->ops.push_back(o);
      }
    }
    // The 3x3, double_3x3_1 and pool_proj layers only depend on the fused 1x1 group: their convs are issued back to
    // back and they share ONE batched BN finalize / apply (forward) and BN-backward launch set.
    int mc[kMaxParts], mp[kMaxParts], nm = 0;
    int pool_in = x;
    if (B.pool == 1) {   // 5b: 3x3 / stride-1 max pool of the block input feeds pool_proj (not linear: stays in front)
      const int XP = add_buf(P, h, w, B.cin);
      pool_idx = add_pool(P, 1, x, XP, 0, 1, 1);
      pool_in = XP;
    }
    {
      std::string n = pre + "_3x3";
      int co = B.c3, db = O, dc = B.c1;
      mc[nm] = c3 = add_conv(P, 1, &n, &co, B.c3r, 3, B.stride, 1, T1, &db, &dc, false);
      P->convs[mc[nm]].slot = nm;
      P->convs[mc[nm]].slot_b = 2;
      mp[nm++] = 0;
    }
    {
      std::string n = pre + "_double_3x3_1";
      int co = B.cd1, db = T3, dc = 0;
      mc[nm] = cd1 = add_conv(P, 1, &n, &co, B.cdr, 3, 1, 1, T2, &db, &dc, false);
      P->convs[mc[nm]].slot = nm;
      P->convs[mc[nm]].slot_b = 1;
      P->convs[mc[nm]].pair_prev = mc[nm - 1];
      P->convs[mc[nm - 1]].pair_next = mc[nm];
      mp[nm++] = 0;
    }
    if (B.pool == 2) {
      if (pool_out(h, 3, 2, 0, true) != oh || pool_out(w, 3, 2, 0, true) != ow) return false;
      pool_idx = add_pool(P, 1, x, O, B.c1 + B.c3 + B.cd2, 2, 0);
    } else if (B.pool == 0) {
      P->convs[g].parts[g_pp].slot = nm;
      P->convs[g].parts[g_pp].slot_b = 3;
      mc[nm] = g;
      mp[nm++] = g_pp;
    } else {
      std::string n = pre + "_pool_proj";
      int co = B.cp, db = O, dc = B.c1 + B.c3 + B.cd2;
      mc[nm] = cpp = add_conv(P, 1, &n, &co, B.cin, 1, 1, 0, pool_in, &db, &dc, false);
      P->convs[mc[nm]].slot = nm;
      P->convs[mc[nm]].slot_b = 3;
      mp[nm++] = 0;
    }
    const int bn_mid = add_bn(P, nm, mc, mp);
    {
      std::string n = pre + "_double_3x3_2";
      int co = B.cd2, db = O, dc = B.c1 + B.c3;
      cd2 = add_conv(P, 1, &n, &co, B.cd1, 3, B.stride, 1, T3, &db, &dc, false);
      bn_d2 = add_bn_conv(P, cd2);
    }
    {
      // what can ride: a member whose destination is the block's OUTPUT buffer is read by nothing inside the block
      tbn_backbone_plan::BlockRiders R;
      R.bn_g = bn_g;
      R.bn_mid = bn_mid;
      R.bn_d2 = bn_d2;
      R.c3 = c3;
      R.cd2 = cd2;
      R.g_defer = R.mid_defer = 0;
      const BnStep& sg = P->bns[bn_g];
      for (int k = 0; k < sg.n; ++k)
        if (P->convs[sg.conv[k]].parts[sg.part[k]].dst_buf == O) R.g_defer |= 1u << k;
      const BnStep& sm = P->bns[bn_mid];
      for (int k = 0; k < sm.n; ++k)
        if (P->convs[sm.conv[k]].parts[sm.part[k]].dst_buf == O) R.mid_defer |= 1u << k;
      P->riders.push_back(R);
    }
    {
      // branch-mode program of this block (see tbn_backbone_plan::ops_b).  Scratch slots: launch-stream layers keep 0 / 1
      // (1x1 group 0, double_3x3_1 1, double_3x3_2 0), side-stream layers take 2 (3x3) and 3 (pool_proj).
      auto push = [&](int kind, int idx, int part, int side) {
        Op o = {kind, idx, part, side};
        P->ops_b.push_back(o);
      };
      push(OP_CONV, g, 0, 0);
      push(OP_BN, bn_g, 0, 0);
      push(OP_FORK, 0, 0, 0);
      int sc[kMaxParts], sp[kMaxParts], sn = 0;
      sc[sn] = c3;
      sp[sn++] = 0;
      if (B.pool == 1) push(OP_POOL, pool_idx, 0, 1);          // 5b: 3x3 / stride-1 max pool of the block input
      if (g_pp >= 0) {
        push(OP_PREPOOL, g, g_pp, 1);
        sc[sn] = g;
        sp[sn++] = g_pp;
      }
      push(OP_CONV, c3, 0, 1);
      if (cpp >= 0) {
        push(OP_CONV, cpp, 0, 1);
        sc[sn] = cpp;
        sp[sn++] = 0;
      }
      if (B.pool == 2) push(OP_POOL, pool_idx, 0, 1);          // 3c / 4e: pass-through max pool into the concat slice
      push(OP_BN, add_bn_only(P, sn, sc, sp, 2), 0, 1);
      push(OP_CONV, cd1, 0, 0);
      {
        const int z = 0;
        push(OP_BN, add_bn_only(P, 1, &cd1, &z, 1), 0, 0);
      }
      push(OP_CONV, cd2, 0, 0);
      push(OP_BN, bn_d2, 0, 0);
      push(OP_JOIN, 0, 0, 0);
    }
    x = O;
    h = oh;
    w = ow;
  }
  P->out_buf = x;
  P->bn_block.assign(P->bns.size(), -1);
  for (size_t b = 0; b < P->riders.size(); ++b) {
    P->bn_block[P->riders[b].bn_g] = P->bn_block[P->riders[b].bn_mid] = P->bn_block[P->riders[b].bn_d2] = (int)b;
  }

  // backward write order: walk ops in reverse, first writer of a d-buffer overwrites, later ones add.  The LAST
  // writer holds the final gradient in its epilogue.
  std::vector<char> written(P->bufs.size(), 0);
  std::vector<int> last_conv(P->bufs.size(), -1);   // conv whose dgrad writes d(buf) last; -1: none / a pool
  for (int i = (int)P->ops.size() - 1; i >= 0; --i) {
    const Op& o = P->ops[i];
    if (o.kind == OP_CONV) {
      Conv& c = P->convs[o.idx];
      if (c.need_dgrad) {
        c.dgrad_accum = written[c.inbuf] != 0;
        written[c.inbuf] = 1;
        last_conv[c.inbuf] = o.idx;
      }
    } else if (o.kind == OP_POOL) {
      Pool& p = P->pools[o.idx];
      p.bwd_accum = written[p.inbuf] != 0;
      written[p.inbuf] = 1;
      last_conv[p.inbuf] = -1;
    }
  }

  // the branch-mode program reorders the layers of a block: it must leave every gradient buffer with the same first
  // (overwriting) and last (reduce-fusing) writer as the serial program, whose flags the kernels are launched with
  {
    std::vector<char> w2(P->bufs.size(), 0);
    std::vector<int> last2(P->bufs.size(), -1);
    bool same = true;
    for (int i = (int)P->ops_b.size() - 1; i >= 0; --i) {
      const Op& o = P->ops_b[i];
      if (o.kind == OP_CONV) {
        const Conv& c = P->convs[o.idx];
        if (c.need_dgrad) {
          same = same && (c.dgrad_accum == (w2[c.inbuf] != 0));
          w2[c.inbuf] = 1;
          last2[c.inbuf] = o.idx;
        }
      } else if (o.kind == OP_POOL) {
        const Pool& q = P->pools[o.idx];
        same = same && (q.bwd_accum == (w2[q.inbuf] != 0));
        w2[q.inbuf] = 1;
        last2[q.inbuf] = -1;
      }
    }
    if (!same || last2 != last_conv) P->ops_b.clear();   // never expected: branch mode is then simply unavailable
  }

  // conv -> BN -> ReLU -> max pool with no other reader of the BN output (the stem: conv1 -> pool1, conv2_3x3 -> pool2):
  // in training the pool runs inside the BN apply and its backward inside the BN backward, so the full-resolution z
  // and dz tensors (the largest of the network) are never written or re-read.
  std::vector<int> readers(P->bufs.size(), 0);
  for (auto& c : P->convs) ++readers[c.inbuf];
  for (auto& q : P->pools) ++readers[q.inbuf];
  for (size_t pi = 0; pi < P->pools.size(); ++pi) {
    Pool& q = P->pools[pi];
    if (q.kind != 1 || q.bwd_accum || readers[q.inbuf] != 1 || q.inbuf == P->out_buf) continue;
    for (auto& c : P->convs)
      if (c.nparts == 1 && c.parts[0].dst_buf == q.inbuf && c.parts[0].dst_choff == 0 && c.cout == P->bufs[q.inbuf].C) {
        c.fuse_pool = (int)pi;
        q.fused = true;
      }
  }

  // BN-backward reduce in the epilogue of the data gradient that finishes dz: every BN layer whose output buffer gets
  // its final gradient from a conv's dgrad (not from outside, not through a fused pool).  Stride-2 dgrads (parity
  // phases) take part as well.  The reduce segments of a conv must start on 32-column boundaries (epilogue sub-tiles).
  for (size_t ci = 0; ci < P->convs.size(); ++ci) {
    Conv& f = P->convs[ci];
    if (!f.need_dgrad || last_conv[f.inbuf] != (int)ci || f.inbuf == P->out_buf) continue;
    struct Cand { int conv, part, choff; };
    std::vector<Cand> cand;
    bool ok = true;
    for (size_t cj = 0; cj < P->convs.size(); ++cj) {
      const Conv& c = P->convs[cj];
      for (int k = 0; k < c.nparts; ++k)
        if (c.parts[k].dst_buf == f.inbuf) {
          if (c.fuse_pool >= 0) ok = false;
          cand.push_back({(int)cj, k, c.parts[k].dst_choff});
        }
    }
    if (!ok || cand.empty() || (int)cand.size() > kMaxParts) continue;
    for (size_t a = 0; a < cand.size(); ++a)
      for (size_t b = a + 1; b < cand.size(); ++b)
        if (cand[b].choff < cand[a].choff) std::swap(cand[a], cand[b]);
    for (auto& cd : cand)
      if (cd.choff % 32 != 0) ok = false;
    if (!ok) continue;
    f.nred = (int)cand.size();
    for (int k = 0; k < f.nred; ++k) {
      f.red_conv[k] = cand[k].conv;
      f.red_part[k] = cand[k].part;
      P->convs[cand[k].conv].parts[cand[k].part].red_src = (int)ci;
    }
  }
  return true;
}

// Timing diagnostics only (-DTBN_DIAG=1 build, never shipped): TBN_DIAG_SKIP=<bit mask> drops kernel groups
// (2 forward BN finalize + apply, 4 pools, 8 BN backward) to measure what each costs the step.
#ifndef TBN_DIAG
#define TBN_DIAG 0
#endif
static inline bool diag_skip(int bit) {
#if TBN_DIAG
  static const int mask = getenv("TBN_DIAG_SKIP") ? atoi(getenv("TBN_DIAG_SKIP")) : 0;
  return (mask & bit) != 0;
#else
  (void)bit;
  return false;
#endif
}
// TBN_DIAG_FOLD=1 (diagnostic build only): the 3x3 / stride-1 layers apply an identity "BN apply + ReLU" (scale 1, shift 0)
// to their input while staging it (LDS-halo forward / data gradient) and in the weight gradient's x operand -- the VALU cost
// of folding the producer's BN apply into the consumers, with unchanged results (their inputs are post-ReLU already)
static inline bool diag_fold() {
#if TBN_DIAG
  static const int on = getenv("TBN_DIAG_FOLD") ? atoi(getenv("TBN_DIAG_FOLD")) : 0;
  return on != 0;
#else
  return false;
#endif
}
void plan_memory(tbn_backbone_plan* P) {
  const size_t R = P->frames;
  size_t off = 0;
  auto take = [&](size_t n) {
    size_t o = off;
    off += (n + 63) / 64 * 64;  // 256-B aligned float regions
    return o;
  };
  for (size_t i = 0; i < P->bufs.size(); ++i) {
    Buf& b = P->bufs[i];
    b.off = i == 0 ? take(R * P->stem_H * P->stem_W * P->cp) : take(R * b.H * b.W * b.C);
  }
  P->x0_off = P->bufs[0].off;
  P->stats_off = take(4 * P->chan_floats);  // mean | rstd | scale | shift
  // per-layer tiles and scratch sizes
  size_t partial = 0, wsplit = 0, wtf = 0;
  for (auto& c : P->convs) {
    const int M = (int)(R * c.outH * c.outW);
    const int K = c.stem ? P->stem_K : c.k * c.k * c.cin;
    tbn_conv_pick_tile(M, c.cout, K, &c.ft[0].mt, &c.ft[0].nt);
    c.ft[1].mt = c.ft[0].mt;
    c.ft[1].nt = c.ft[0].nt;
    size_t a = (size_t)cdiv(M, M <= kSk4MaxRows ? 32 : 128) * 2 * c.cout;  // worst case (mt = 1): autotune may pick any tile
    if (a > partial) partial = a;
    for (int k = 0; k < c.nparts; ++k) {
      size_t bparts = (size_t)tbn_bn_bwd_parts(M, c.parts[k].cout) * 2 * c.parts[k].cout;
      if (bparts > partial) partial = bparts;
    }
    const int taps = c.stem ? 1 : c.k * c.k, ci = c.stem ? P->stem_rows * P->kw : c.cin;
    size_t ws = tbn_wgrad_workspace_floats(M, c.cout, ci, taps);
    if (ws > wsplit) wsplit = ws;
    if (c.need_dgrad) {
      const int Md = (int)(R * c.inH * c.inW);
      tbn_conv_pick_tile(Md, c.cin, c.k * c.k * c.cout, &c.d_mt, &c.d_nt);
    }
  }
  // flipped / transposed copy of every data-gradient weight, at the layer's own offset
  wtf = P->weight_floats;
  memset(&P->flip, 0, sizeof(P->flip));
  for (auto& c : P->convs)
    if (c.need_dgrad && P->flip.n < 64) {
      FlipTab& f = P->flip;
      f.w_off[f.n] = (int)c.w_off;
      f.cout[f.n] = (short)c.cout;
      f.cin[f.n] = (short)c.cin;
      f.taps[f.n] = (short)(c.k * c.k);
      f.blk0[f.n + 1] = f.blk0[f.n] + cdiv(c.cin, 32) * cdiv(c.cout, 32);   // one workgroup per 32 x 32 tile, all taps
      ++f.n;
    }
  P->partial_floats = partial;
  P->wsplit_floats = wsplit;
  P->wt_floats = wtf;
  P->partial_off = take(TBN_BN_MAXL * partial);   // one region per member of a batched BN step
  P->wpack_off = take((size_t)64 * P->stem_K);
  for (auto& c : P->convs)   // raw / pooled conv output of the pool-after-conv layers: needed in eval too
    for (int k = 0; k < c.nparts; ++k)
      if (c.parts[k].pooled) {
        c.parts[k].yraw_off = take(R * c.outH * c.outW * c.parts[k].cout);
        c.parts[k].y2_off = take(R * c.outH * c.outW * c.parts[k].cout);
      }
  P->eval_floats = off;
  // training-only regions
  for (auto& c : P->convs) c.y_off = take(R * c.outH * c.outW * c.cout);
  for (size_t i = 1; i < P->bufs.size(); ++i) {
    if ((int)i == P->out_buf) continue;  // gradient of the final feature map is supplied by the caller
    P->bufs[i].doff = take(R * P->bufs[i].H * P->bufs[i].W * P->bufs[i].C);
  }
  for (auto& c : P->convs)   // BN-backward partials filled by a data-gradient epilogue: live until that layer's BN backward
    for (int k = 0; k < c.nparts; ++k)
      if (c.parts[k].red_src >= 0) {
        const Buf& db = P->bufs[c.parts[k].dst_buf];
        const int drows = (int)(R * db.H * db.W);
        c.parts[k].bpart_off = take(((size_t)cdiv(drows, drows <= kSk4MaxRows ? 32 : 128) + 4) * 2 * c.parts[k].cout);
      }
  P->coef_off = take(TBN_BN_MAXL * 3 * 1024);
  P->diag_fold_off = take(2 * 2048);
  P->wsplit_off = take(wsplit);
  P->wt_off = take(wtf);
  P->dwpack_off = take((size_t)64 * P->stem_rows * P->kw);
  size_t bytes = off * sizeof(float);
  P->argmax_bytes_off = bytes;
  for (auto& p : P->pools)
    if (p.kind == 1) {
      const Buf& ob = P->bufs[p.outbuf];
      const Buf& ib = P->bufs[p.inbuf];
      p.argmax_off = bytes;
      bytes += align_up(R * ob.H * ob.W * ib.C, 256);
    }
  P->total_bytes_train = bytes;
  P->total_bytes_eval = P->eval_floats * sizeof(float);
}

}  // namespace

extern "C" {

int tbn_backbone_plan_create(int in_channels, int frames, int height, int width, tbn_backbone_plan** out) {
  TBN_REQUIRE(out != nullptr, "plan_create: null out");
  TBN_REQUIRE(in_channels >= 1 && in_channels <= 16 && frames >= 1 && height >= 32 && width >= 32,
              "plan_create: unsupported shape (C=%d, frames=%d, %dx%d)", in_channels, frames, height, width);
  TBN_REQUIRE((long)frames * height * width < (1l << 31) / 4, "plan_create: too many pixels per call (chunk the batch)");
  tbn_backbone_plan* P = new tbn_backbone_plan();
  P->cin0 = in_channels;
  P->frames = frames;
  P->H = height;
  P->W = width;
  if (!build_graph(P) || P->bufs[P->out_buf].H < 1 || P->bufs[P->out_buf].W < 1) {
    delete P;
    tbn_set_error("plan_create: %dx%d input is not a valid BN-Inception size (the stride-2 conv branches and the "
                  "ceil-mode pass-through max pool of inception_3c / 4e disagree; the reference's torch.cat raises)",
                  height, width);
    return TBN_ERR_UNSUPPORTED;
  }
  {
    int nd = 0;
    for (auto& c : P->convs) nd += c.need_dgrad ? 1 : 0;
    if (nd > 64) {
      delete P;
      tbn_set_error("plan_create: %d data-gradient layers exceed the flip table (64)", nd);
      return TBN_ERR_UNSUPPORTED;
    }
  }
  {
    // every tensor a kernel addresses through ONE buffer descriptor must stay below 2 GiB (32-bit byte offsets with the
    // hardware range check): refuse here, on the host, what would otherwise fail at some launch in the middle of a pass.
    // Training cannot chunk the frames (batch statistics); eval callers chunk (BNInception.eval_chunk).
    size_t worst = (size_t)frames * P->stem_H * P->stem_W * P->cp;                 // the bordered input image
    const char* what = "network input";
    for (size_t i = 1; i < P->bufs.size(); ++i) {
      const size_t n = (size_t)frames * P->bufs[i].H * P->bufs[i].W * P->bufs[i].C;
      if (n > worst) {
        worst = n;
        what = "an activation buffer";
      }
    }
    for (auto& c : P->convs) {
      const size_t n = (size_t)frames * c.outH * c.outW * c.cout;
      if (n > worst) {
        worst = n;
        what = c.parts[0].name.c_str();
      }
    }
    if (worst * sizeof(float) >= (1ull << 31)) {
      tbn_set_error("plan_create: %d frames of %dx%d make a %.2f GiB tensor (%s); one engine call addresses at most 2 GiB per "
                    "tensor -- use fewer frames per call (eval: chunk them; training: a smaller per-GPU batch)",
                    frames, height, width, (double)(worst * sizeof(float)) / (1ull << 30), what);
      delete P;
      return TBN_ERR_UNSUPPORTED;
    }
  }
  plan_memory(P);
  *out = P;
  return TBN_OK;
}

void tbn_backbone_plan_destroy(tbn_backbone_plan* p) {
  if (!p) return;
  for (int i = 0; i < p->n_ev; ++i) (void)hipEventDestroy(p->ev[i]);
  delete p;
}

int tbn_backbone_num_convs(const tbn_backbone_plan* P) {
  int n = 0;
  for (auto& c : P->convs) n += c.nparts;
  return n;
}

int tbn_backbone_conv_info(const tbn_backbone_plan* P, int idx, tbn_conv_info* info) {
  TBN_REQUIRE(info != nullptr, "conv_info: null info");
  int n = 0;
  for (auto& c : P->convs) {
    size_t w = c.w_off;
    for (int i = 0; i < c.nparts; ++i) {
      if (n == idx) {
        memset(info, 0, sizeof(*info));
        snprintf(info->name, sizeof(info->name), "%s", c.parts[i].name.c_str());
        info->cin = c.cin;
        info->cout = c.parts[i].cout;
        info->ksize = c.k;
        info->stride = c.stride;
        info->pad = c.pad;
        info->weight_offset = w;
        info->channel_offset = c.parts[i].c_off;
        return TBN_OK;
      }
      w += (size_t)c.parts[i].cout * c.k * c.k * c.cin;
      ++n;
    }
  }
  tbn_set_error("conv_info: index %d out of range", idx);
  return TBN_ERR_ARG;
}

// debugging / per-layer parity tests: where one conv's tensors live inside the workspace.
// kind 0: z = relu(bn(conv)) destination slice; 1: BN input y (after backward: dy);
// 2: gradient wrt z (for the final block the gradient is external: -1); 3: the conv's whole INPUT buffer (a block's
// concat buffer / a pool output).  offset in floats.
int tbn_backbone_tensor_info(const tbn_backbone_plan* P, const char* conv_name, int kind, long* offset, int* rows,
                             int* cols, int* ld) {
  for (auto& c : P->convs)
    for (int i = 0; i < c.nparts; ++i) {
      const Part& q = c.parts[i];
      if (q.name != conv_name) continue;
      const Buf& db = P->bufs[q.dst_buf];
      *rows = P->frames * c.outH * c.outW;
      *cols = q.cout;
      if (kind == 3) {
        TBN_REQUIRE(!c.stem, "tensor_info: the stem reads the bordered space-to-depth image, not an NHWC buffer");
        const Buf& ib = P->bufs[c.inbuf];
        *offset = (long)ib.off;
        *rows = P->frames * c.inH * c.inW;
        *cols = *ld = ib.C;
        return TBN_OK;
      }
      if (kind == 4) {   // training-mode BN coefficients: mean | rstd | scale | shift rows
        *offset = (long)(P->stats_off + q.c_off);
        *rows = 4;
        *ld = (int)P->chan_floats;
        return TBN_OK;
      }
      if (kind == 1) {
        *offset = (long)(q.pooled ? q.y2_off : c.y_off + q.col0);
        *ld = q.pooled ? q.cout : c.cout;
      } else if (kind == 0) {
        if (c.fuse_pool >= 0) {
          tbn_set_error("tensor_info: z of '%s' is never written (its max pool runs inside the BN apply): rebuild it "
                        "from kinds 1 and 4", conv_name);
          return TBN_ERR_UNSUPPORTED;
        }
        *offset = (long)(db.off + q.dst_choff);
        *ld = db.C;
      } else {
        *offset = q.dst_buf == P->out_buf ? -1 : (long)(db.doff + q.dst_choff);
        *ld = db.C;
      }
      return TBN_OK;
    }
  tbn_set_error("tensor_info: unknown conv '%s'", conv_name);
  return TBN_ERR_ARG;
}

int tbn_backbone_launch_info(const tbn_backbone_plan* P, const char* conv_name, int training, int* out16) {
  TBN_REQUIRE(P && conv_name && out16, "launch_info: null argument");
  for (auto& c : P->convs)
    for (int i = 0; i < c.nparts; ++i) {
      if (c.parts[i].name != conv_name) continue;
      const Conv::FwdTune& T = c.ft[training ? 1 : 0];
      const int f[8] = {T.halo, T.mt, T.nt, T.stages, T.pair ? 1 : 0, T.p_variant, T.p_mt, T.p_nt};
      const int d[8] = {c.d_halo, c.d_mt, c.d_nt, c.d_stages, c.pair_dgrad ? 1 : 0, c.pd_variant, c.pd_mt, c.pd_nt};
      for (int k = 0; k < 8; ++k) {
        out16[k] = f[k];
        out16[8 + k] = (training && c.need_dgrad) ? d[k] : 0;
      }
      return TBN_OK;
    }
  tbn_set_error("launch_info: unknown conv '%s'", conv_name);
  return TBN_ERR_ARG;
}

// ---- tuned launch choices as a relocatable blob (host memory): what tbn_backbone_autotune decides, nothing that depends
// on addresses.  Layout: 8 int32 header {magic, version, in_channels, frames, H, W, number of GEMMs, ints per GEMM} followed
// by kPlanInts int32 per GEMM in plan order.
namespace {
constexpr int kPlanMagic = 0x54424e50;   // "TBNP"
constexpr int kPlanVersion = 1;
constexpr int kPlanInts = 26;
void plan_pack(const Conv& c, int* o) {
  int k = 0;
  for (int m = 0; m < 2; ++m) {
    const Conv::FwdTune& T = c.ft[m];
    o[k++] = T.mt; o[k++] = T.nt; o[k++] = T.stages; o[k++] = T.halo;
    o[k++] = T.pair ? 1 : 0; o[k++] = T.p_variant; o[k++] = T.p_mt; o[k++] = T.p_nt;
  }
  o[k++] = c.d_mt; o[k++] = c.d_nt; o[k++] = c.d_stages; o[k++] = c.d_halo;
  o[k++] = c.pair_dgrad ? 1 : 0; o[k++] = c.pd_variant; o[k++] = c.pd_mt; o[k++] = c.pd_nt;
  o[k++] = c.w_mt; o[k++] = c.w_nt;
}
bool tile_ok(int mt, int nt) { return mt >= 1 && mt <= 2 && nt >= 1 && nt <= 4; }
}  // namespace

size_t tbn_backbone_plan_export_bytes(const tbn_backbone_plan* P) {
  return P ? sizeof(int) * (8 + (size_t)kPlanInts * P->convs.size()) : 0;
}

int tbn_backbone_plan_export(const tbn_backbone_plan* P, void* buf, size_t bytes) {
  TBN_REQUIRE(P && buf, "plan_export: null argument");
  TBN_REQUIRE(bytes >= tbn_backbone_plan_export_bytes(P), "plan_export: buffer too small (%zu < %zu bytes)", bytes,
              tbn_backbone_plan_export_bytes(P));
  int* o = (int*)buf;
  const int hdr[8] = {kPlanMagic, kPlanVersion, P->cin0, P->frames, P->H, P->W, (int)P->convs.size(), kPlanInts};
  memcpy(o, hdr, sizeof(hdr));
  for (size_t i = 0; i < P->convs.size(); ++i) plan_pack(P->convs[i], o + 8 + kPlanInts * i);
  return TBN_OK;
}

// Adopts the launch choices of a blob written by tbn_backbone_plan_export for the SAME problem (input channels, frames,
// H, W): every replica of a data-parallel job then runs the kernels rank 0 tuned (the reference's nn.DataParallel
// replicas are identical by construction, core/models/model_builder.py:73-75).  Every field is validated against what the
// launchers accept; a blob that fails leaves the plan untouched.
int tbn_backbone_plan_import(tbn_backbone_plan* P, const void* buf, size_t bytes) {
  TBN_REQUIRE(P && buf, "plan_import: null argument");
  TBN_REQUIRE(bytes >= sizeof(int) * 8, "plan_import: truncated blob (%zu bytes)", bytes);
  const int* in = (const int*)buf;
  TBN_REQUIRE(in[0] == kPlanMagic && in[1] == kPlanVersion, "plan_import: not a plan blob of this library (magic %08x, version %d)",
              in[0], in[1]);
  TBN_REQUIRE(in[2] == P->cin0 && in[3] == P->frames && in[4] == P->H && in[5] == P->W,
              "plan_import: blob is for (C=%d, frames=%d, %dx%d), this plan for (C=%d, frames=%d, %dx%d)", in[2], in[3], in[4],
              in[5], P->cin0, P->frames, P->H, P->W);
  TBN_REQUIRE(in[6] == (int)P->convs.size() && in[7] == kPlanInts && bytes >= tbn_backbone_plan_export_bytes(P),
              "plan_import: blob holds %d GEMMs x %d ints (%zu bytes), expected %zu x %d", in[6], in[7], bytes, P->convs.size(),
              kPlanInts);
  for (size_t i = 0; i < P->convs.size(); ++i) {
    const int* q = in + 8 + kPlanInts * i;
    const Conv& c = P->convs[i];
    bool ok = true;
    for (int m = 0; m < 2; ++m) {
      const int* f = q + 8 * m;
      ok = ok && tile_ok(f[0], f[1]) && f[2] >= 0 && f[2] <= 2 && f[3] >= 0 && f[3] <= 3 && (f[4] == 0 || f[4] == 1) &&
           f[5] >= 0 && f[5] <= 2 && tile_ok(f[6], f[7]) && f[6] <= 2 && f[7] <= 2;
      ok = ok && !(f[4] == 1 && c.pair_next < 0);                        // a pair decision lives on a pair's first member
      ok = ok && !(c.stem && f[3] != 0);                                 // the stem runs the packed-row kernel only
      ok = ok && !(f[3] == 3 && (f[0] > 2 || f[1] > 2));                 // split-K tile kernel: tiles up to (2, 2)
    }
    const int* d = q + 16;
    ok = ok && tile_ok(d[0], d[1]) && d[2] >= 0 && d[2] <= 2 && d[3] >= 0 && d[3] <= 3 && (d[4] == 0 || d[4] == 1) &&
         d[5] >= 0 && d[5] <= 2 && tile_ok(d[6], d[7]) && d[6] <= 2 && d[7] <= 2;
    ok = ok && !(d[4] == 1 && (c.pair_next < 0 || c.stride != 1));
    ok = ok && !(d[3] == 3 && (d[0] > 2 || d[1] > 2 || c.stride != 1));
    ok = ok && !((d[3] == 1 || d[3] == 2) && c.stride != 1);            // parity-phase launches: register-staged kernel
    ok = ok && tbn_wgrad_tile_ok(q[24], q[25]);   // (tbn_wgrad_plan would swap any other value for a tile of its own)
    TBN_REQUIRE(ok, "plan_import: invalid launch choice for GEMM %zu (%s)", i, c.parts[c.nparts - 1].name.c_str());
  }
  for (size_t i = 0; i < P->convs.size(); ++i) {
    const int* q = in + 8 + kPlanInts * i;
    Conv& c = P->convs[i];
    for (int m = 0; m < 2; ++m) {
      Conv::FwdTune& T = c.ft[m];
      const int* f = q + 8 * m;
      T.mt = f[0]; T.nt = f[1]; T.stages = f[2]; T.halo = f[3];
      T.pair = f[4] != 0; T.p_variant = f[5]; T.p_mt = f[6]; T.p_nt = f[7];
    }
    const int* d = q + 16;
    c.d_mt = d[0]; c.d_nt = d[1]; c.d_stages = d[2]; c.d_halo = d[3];
    c.pair_dgrad = d[4] != 0; c.pd_variant = d[5]; c.pd_mt = d[6]; c.pd_nt = d[7];
    c.w_mt = q[24]; c.w_nt = q[25];
  }
  return TBN_OK;
}

// 64-bit FNV-1a over the export blob: equal fingerprints <=> equal launch choices for the same problem
unsigned long long tbn_backbone_plan_fingerprint(const tbn_backbone_plan* P) {
  if (!P) return 0;
  std::vector<int> blob(8 + (size_t)kPlanInts * P->convs.size());
  if (tbn_backbone_plan_export(P, blob.data(), blob.size() * sizeof(int)) != TBN_OK) return 0;
  unsigned long long h = 1469598103934665603ull;
  const unsigned char* b = (const unsigned char*)blob.data();
  for (size_t i = 0; i < blob.size() * sizeof(int); ++i) {
    h ^= b[i];
    h *= 1099511628211ull;
  }
  return h;
}

size_t tbn_backbone_weight_floats(const tbn_backbone_plan* P) { return P->weight_floats; }
size_t tbn_backbone_channel_floats(const tbn_backbone_plan* P) { return P->chan_floats; }
size_t tbn_backbone_workspace_bytes(const tbn_backbone_plan* P, int training) {
  return training ? P->total_bytes_train : P->total_bytes_eval;
}
int tbn_backbone_num_streams(const tbn_backbone_plan* P) { return P->ops_b.empty() ? 1 : 2; }
int tbn_backbone_rider_launches(const tbn_backbone_plan* P, int* forward, int* backward) {
  TBN_REQUIRE(P != nullptr, "rider_launches: null plan");
  if (forward) *forward = P->rider_launches[0];
  if (backward) *backward = P->rider_launches[1];
  return TBN_OK;
}
int tbn_backbone_out_shape(const tbn_backbone_plan* P, int* h, int* w, int* c) {
  const Buf& b = P->bufs[P->out_buf];
  if (h) *h = b.H;
  if (w) *w = b.W;
  if (c) *c = b.C;
  return TBN_OK;
}

}  // extern "C"

namespace {

// forward-conv launch parameters of one GEMM (shared by forward and autotune); output segments are set by the caller
void fill_fwd(const tbn_backbone_plan* P, const Conv& c, int training, float* ws, const float* weight, int R, ConvP* pp) {
  ConvP& p = *pp;
  const Buf& ib = P->bufs[c.inbuf];
  memset(&p, 0, sizeof(p));
  p.in = ws + ib.off;
  p.in_ld = ib.C;
  p.N = R;
  p.H = c.inH;
  p.W = c.inW;
  p.OH = c.outH;
  p.OW = c.outW;
  p.Cout = c.cout;
  p.stride = c.stride;
  p.pad = c.pad;
  p.up = 1;
  p.M = R * c.outH * c.outW;
  p.bias = nullptr;  // training: cancels in the batch-stat BN (finalize adds it to running_mean); eval: folded into shift
  p.alg_flops = 2.0 * p.M * (double)c.cout * c.k * c.k * c.cin;
  if (c.stem) {
    p.wt = ws + P->wpack_off;
    p.Cin = P->kw;
    p.R = P->stem_rows;
    p.S = 1;
    p.K = P->stem_K;
    p.cp = p.in_ld = P->cp;
    p.H = P->stem_H;          // the 4-row / stride-1 conv on the bordered space-to-depth image
    p.W = P->stem_W;
    p.stride = P->stem_stride;
    p.pad = P->stem_pad;
  } else {
    p.wt = weight + c.w_off;
    p.Cin = c.cin;
    p.R = p.S = c.k;
    p.K = c.k * c.k * c.cin;
  }
  p.stages = c.ft[training ? 1 : 0].stages;
  p.halo = c.ft[training ? 1 : 0].halo;
  if (diag_fold() && training && !c.stem && c.k == 3 && c.stride == 1) {
    p.fold_scale = ws + P->diag_fold_off;
    p.fold_shift = ws + P->diag_fold_off + 2048;
  }
}

// Forward epilogue of one GEMM (fill_fwd first).  Training: the raw (bias-free) conv output of every part goes to the
// layer's y buffer, the per-channel statistics partials to scratch slot `slot`.  Eval: running-stat BN + ReLU folded
// into the epilogue, every part straight into its concat slice; a pooled part (pool_proj) leaves the bare conv output
// for its average pool.
void fill_fwd_epilogue(const tbn_backbone_plan* P, const Conv& c, int training, float* ws, int slot, ConvP* pp) {
  ConvP& p = *pp;
  if (training) {
    p.mode = CONV_EPI_STATS;
    p.nseg = 1;
    p.seg[0].ptr = ws + c.y_off;
    p.seg[0].ld = c.cout;
    p.seg[0].col_begin = 0;
    p.stat_partial = ws + P->partial_off + (size_t)slot * P->partial_floats;
    return;
  }
  float* scale = ws + P->stats_off + 2 * P->chan_floats;   // mean | rstd | scale | shift
  p.mode = CONV_EPI_EVAL;
  p.scale = scale + c.c_off;
  p.shift = scale + P->chan_floats + c.c_off;
  p.nseg = c.nparts;
  for (int i = 0; i < c.nparts; ++i) {
    const Part& q = c.parts[i];
    const Buf& db = P->bufs[q.dst_buf];
    p.seg[i].ptr = q.pooled ? ws + q.yraw_off : ws + db.off + q.dst_choff;
    p.seg[i].ld = q.pooled ? q.cout : db.C;
    p.seg[i].col_begin = q.col0;
    if (q.pooled) p.raw_seg1 = i + 1;
  }
}

// The tuned launch choices of one GEMM kind of a conv, as the walks read them: the forward in eval / training mode
// (= the index into Conv::ft) or the data gradient.
enum { GEMM_FWD_EVAL = 0, GEMM_FWD_TRAIN = 1, GEMM_DGRAD = 2 };
struct Tuned {
  int halo, mt;   // single launch: kernel variant and M tile
  bool pair;      // sibling-pair decision (held by the first member)
  int p_mt;       // M tile of the pair launch
};
Tuned tuned(const Conv& c, int gemm) {
  if (gemm == GEMM_DGRAD) return {c.d_halo, c.d_mt, c.pair_dgrad, c.pd_mt};
  const Conv::FwdTune& T = c.ft[gemm];
  return {T.halo, T.mt, T.pair, T.p_mt};
}
// How conv `c` is issued in a walk: 0 as its own launch, 1 as the FIRST member of a sibling-pair launch (it issues the
// launch for both), 2 as the SECOND member (it ran with its sibling).  Branch mode (`br`) never pairs, whatever the plan
// holds: the siblings belong to different chains there -- 3x3 on the side stream, double_3x3_1 on the launch stream --
// and one grid cannot run on two streams.
int pair_role(const tbn_backbone_plan* P, const Conv& c, int gemm, bool br) {
  if (br) return 0;
  if (c.pair_next >= 0 && tuned(c, gemm).pair) return 1;
  if (c.pair_prev >= 0 && tuned(P->convs[c.pair_prev], gemm).pair) return 2;
  return 0;
}
// M rows per workgroup tile of the launch that wrote the partial rows of conv `c` (forward: BN statistics, data gradient:
// fused BN-backward reduce) = rows summed into one partial row.  A pair launch has its own tile, 128-row kernels only.
int writer_rows(const tbn_backbone_plan* P, const Conv& c, int gemm, bool br) {
  const int role = pair_role(P, c, gemm, br);
  if (role == 0) return tile_rows(tuned(c, gemm).halo, tuned(c, gemm).mt);
  return 128 * tuned(role == 1 ? c : P->convs[c.pair_prev], gemm).p_mt;
}

// data-gradient launch parameters of one GEMM: conv of dy with flipped / transposed weights (parity phases for
// stride 2), plus the fused BN-backward reduce of the layers whose dz it finishes
void fill_dgrad(const tbn_backbone_plan* P, const Conv& c, float* ws, int R, ConvP* pp) {
  ConvP& p = *pp;
  const Buf& ib = P->bufs[c.inbuf];
  memset(&p, 0, sizeof(p));
  p.in = ws + c.y_off;
  p.in_ld = c.cout;
  p.wt = ws + P->wt_off + c.w_off;
  p.N = R;
  p.H = c.outH;
  p.W = c.outW;
  p.OH = c.inH;
  p.OW = c.inW;
  p.Cin = c.cout;
  p.Cout = c.cin;
  p.R = p.S = c.k;
  p.stride = 1;
  p.pad = c.k - 1 - c.pad;
  p.up = c.stride;      // stride-2 layers: the four parity phases in one launch
  p.M = R * c.inH * c.inW;
  p.K = c.k * c.k * c.cout;
  p.alg_flops = 2.0 * R * c.outH * c.outW * (double)c.cout * c.k * c.k * c.cin;  // = forward count (zero-insertion not counted)
  p.mode = CONV_EPI_PLAIN;
  p.flags = c.dgrad_accum ? CONV_FLAG_ACCUM : 0;
  p.nseg = 1;
  p.seg[0].ptr = ws + ib.doff;
  p.seg[0].ld = ib.C;
  p.seg[0].col_begin = 0;
  p.stages = c.d_stages;
  p.halo = c.d_halo;
  p.nred = c.nred;
  p.red_chan = (int)P->chan_floats;
  for (int k = 0; k < c.nred; ++k) {
    const Conv& pc = P->convs[c.red_conv[k]];
    const Part& q = pc.parts[c.red_part[k]];
    RedSeg& r = p.red[k];
    r.y = q.pooled ? ws + q.y2_off : ws + pc.y_off + q.col0;
    r.y_ld = q.pooled ? q.cout : pc.cout;
    r.partial = ws + q.bpart_off;
    r.stats = ws + P->stats_off;
    r.col_begin = q.dst_choff;
    r.C = q.cout;
    r.c_off = (int)q.c_off;
  }
  if (c.nred > 0 && p.red[0].col_begin != 0) {
    // columns in front of the first BN layer (none in this graph) would need a leading empty segment
    p.nred = 0;
  }
}

// weight-gradient launch parameters of one conv (shared by backward and autotune)
void fill_wgrad(const tbn_backbone_plan* P, const Conv& c, float* ws, int R, WgradP* wp) {
  const Buf& ib = P->bufs[c.inbuf];
  memset(wp, 0, sizeof(*wp));
  wp->dy = ws + c.y_off;
  wp->dy_ld = c.cout;
  wp->x = ws + ib.off;
  wp->x_ld = ib.C;
  wp->N = R;
  wp->H = c.inH;
  wp->W = c.inW;
  wp->OH = c.outH;
  wp->OW = c.outW;
  wp->Cout = c.cout;
  wp->stride = c.stride;
  wp->pad = c.pad;
  wp->M = R * c.outH * c.outW;
  wp->alg_flops = 2.0 * wp->M * (double)c.cout * c.k * c.k * c.cin;
  wp->mt = c.w_mt;
  wp->nt = c.w_nt;
  if (c.stem) {
    wp->Cin = P->stem_rows * P->kw;
    wp->R = P->stem_rows;
    wp->S = 1;
    wp->taps = 1;
    wp->cp = wp->x_ld = P->cp;
    wp->rl = P->kw;
    wp->H = P->stem_H;
    wp->W = P->stem_W;
    wp->stride = P->stem_stride;
    wp->pad = P->stem_pad;
  } else {
    wp->Cin = c.cin;
    wp->R = wp->S = c.k;
    wp->taps = c.k * c.k;
    if (diag_fold() && c.k == 3) {
      wp->fold_scale = ws + P->diag_fold_off;
      wp->fold_shift = ws + P->diag_fold_off + 2048;
    }
  }
}

// fork / join events of the aux (weight-gradient) and side (branch) streams: created on first use, outside any capture
int ensure_events(tbn_backbone_plan* PM) {
  constexpr int NE = tbn_backbone_plan::kEvents;
  for (int i = PM->n_ev; i < NE; ++i) {
    if (hipEventCreateWithFlags(&PM->ev[i], hipEventDisableTiming) != hipSuccess) {
      tbn_set_error("backbone: hipEventCreate failed");
      return TBN_ERR_LAUNCH;
    }
    PM->n_ev = i + 1;
  }
  return TBN_OK;
}

// whatever is enqueued on `to` from here on runs after everything `from` holds now
void order_after(hipEvent_t e, hipStream_t from, hipStream_t to) {
  (void)hipEventRecord(e, from);
  (void)hipStreamWaitEvent(to, e, 0);
}

// joins the aux (weight-gradient) stream into the launch stream on every exit path of tbn_backbone_backward
struct AuxJoin {
  hipStream_t st, aux;
  hipEvent_t ev;
  bool forked = false;
  ~AuxJoin() {
    if (aux != nullptr && forked) order_after(ev, aux, st);
  }
};

// The side (branch) stream of a walk.  turn(): at a FORK the side stream continues from where the launch stream is, at a
// join the launch stream waits for the side chain of the block.  The destructor joins on every exit path: a TBN_TRY /
// TBN_REQUIRE that returns between a fork and its join would otherwise leave side-stream kernels reading and writing the
// workspace while the caller (seeing the error) frees or reuses it, or enqueues on the launch stream (round-4 advisor)
struct SideJoin {
  hipStream_t st, side;
  hipEvent_t ev;
  bool open = false;   // the side chain of the current block has been forked and not yet joined
  void turn(hipEvent_t e, bool fork) {
    order_after(e, fork ? st : side, fork ? side : st);
    open = fork;
  }
  ~SideJoin() {
    if (side != nullptr && open) order_after(ev, side, st);
  }
};

}  // namespace

extern "C" {

// bf16 weight planes of the backbone (TBN_BACKBONE_CONV_BF16X_ALL): every GEMM the shape rule (tbn_kernels.h) gives to a
// split-bf16 kernel owns a run of records (conv_bf16x.hip) in plan order; off[i] = byte offset of conv i's records,
// -1 = none.  The map width is not asked (see bf16x_3x3_map_ok): a conv2_3x3 on a map wider than 64 stays on the fp32
// kernel and its planes (110592 weights, 0.65 MB of ~40 MB at np 6) are written and never read.
static Bf16xLayer conv_bf16x_layer(const Conv& c) { return c.stem ? BF16X_LAYER_NONE : bf16x_layer_kind(c.k, c.stride, c.pad, c.cin); }
static size_t planes_layout(const tbn_backbone_plan* P, int np, std::vector<long long>* off) {
  size_t total = 0;
  if (off) off->assign(P->convs.size(), -1);
  for (size_t i = 0; i < P->convs.size(); ++i) {
    const Conv& c = P->convs[i];
    if (conv_bf16x_layer(c) == BF16X_LAYER_NONE) continue;
    if (off) (*off)[i] = (long long)total;
    total += tbn_bf16x_planes_bytes((size_t)c.cout * c.k * c.k * c.cin, np);
  }
  return total;
}

size_t tbn_backbone_weight_planes_bytes(const tbn_backbone_plan* P, int np) {
  if (!P || (np != 6 && np != 3)) return 0;
  return planes_layout(P, np, nullptr);
}

int tbn_backbone_split_weights(const tbn_backbone_plan* P, const float* weight, int np, void* planes, void* stream) {
  TBN_REQUIRE(P && weight && planes, "backbone_split_weights: null argument");
  TBN_REQUIRE(np == 6 || np == 3, "backbone_split_weights: np must be 6 (bf16x6) or 3 (bf16x3), got %d", np);
  TBN_REQUIRE((((uintptr_t)weight | (uintptr_t)planes) & 15) == 0, "backbone_split_weights: pointers must be 16-B aligned");
  std::vector<long long> off;
  planes_layout(P, np, &off);
  static thread_local SplitTab tab;
  tab.n = 0;
  for (size_t i = 0; i < P->convs.size(); ++i) {
    if (off[i] < 0) continue;
    const Conv& c = P->convs[i];
    TBN_REQUIRE(split_tab_push(tab, c.w_off, (size_t)off[i], (size_t)c.cout * c.k * c.k * c.cin),
                "backbone_split_weights: more than 64 weight tensors");
  }
  return tbn_launch_bf16x_split(weight, planes, tab, np, (hipStream_t)stream);
}

int tbn_backbone_forward(const tbn_backbone_plan* P, int training, const float* x_nchw,
                         const tbn_backbone_params* prm, void* workspace, size_t workspace_bytes,
                         float** features_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  TBN_REQUIRE(P && x_nchw && prm && workspace && features_out, "backbone_forward: null argument");
  TBN_REQUIRE(workspace_bytes >= tbn_backbone_workspace_bytes(P, training), "backbone_forward: workspace too small");
  TBN_REQUIRE(((uintptr_t)workspace & 255) == 0, "backbone_forward: workspace must be 256-B aligned");
  TBN_REQUIRE((prm->flags & (TBN_BACKBONE_CONV_BF16X6 | TBN_BACKBONE_CONV_BF16X3)) != (TBN_BACKBONE_CONV_BF16X6 | TBN_BACKBONE_CONV_BF16X3),
              "backbone_forward: TBN_BACKBONE_CONV_BF16X6 and _BF16X3 (bf16x math modes) are exclusive");
  // TBN_BACKBONE_CONV_BF16X_ALL: honoured in eval mode beside one of the math flags only
  const bool bf16x_all = !training && (prm->flags & TBN_BACKBONE_CONV_BF16X_ALL) != 0 &&
                         (prm->flags & (TBN_BACKBONE_CONV_BF16X6 | TBN_BACKBONE_CONV_BF16X3)) != 0;
  if (bf16x_all) {
    if (prm->weight_planes == nullptr) {
      tbn_set_error("backbone_forward: TBN_BACKBONE_CONV_BF16X_ALL (bf16x weight planes) needs tbn_backbone_params.weight_planes");
      return TBN_ERR_ARG;
    }
    TBN_REQUIRE(((uintptr_t)prm->weight_planes & 15) == 0, "backbone_forward: bf16x weight_planes must be 16-B aligned");
  }
  float* ws = (float*)workspace;
  const int R = P->frames;
  const int tr = training ? 1 : 0;   // index of the forward launch choices (Conv::ft)
  // branch mode: the caller gave a side stream and nothing is being captured (forks inside a capture: see backward)
  hipStream_t side = (hipStream_t)prm->side_stream;
  if (side == st || P->ops_b.empty()) side = nullptr;
  if (side != nullptr) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) side = nullptr;
  }
  const bool br = side != nullptr;
  tbn_backbone_plan* PM = const_cast<tbn_backbone_plan*>(P);  // event pool only
  if (br) TBN_TRY(ensure_events(PM));
  SideJoin sjoin{st, side, br ? PM->ev[tbn_backbone_plan::kEvents - 2] : nullptr};
  int ev_next = 0;
  float* mean = ws + P->stats_off;
  float* rstd = mean + P->chan_floats;
  float* scale = rstd + P->chan_floats;
  float* shift = scale + P->chan_floats;
  float* wpack = ws + P->wpack_off;

  if (diag_fold() && training) {
    (void)hipMemsetD32Async((hipDeviceptr_t)(ws + P->diag_fold_off), 0x3f800000, 2048, st);
    (void)hipMemsetD32Async((hipDeviceptr_t)(ws + P->diag_fold_off + 2048), 0, 2048, st);
  }
  if (P->stem_mode == 1) {
    TBN_TRY(tbn_launch_nchw_to_nhwc_pad(x_nchw, ws + P->x0_off, R, P->cin0, P->H, P->W, P->stem_H, P->stem_W, st));
    TBN_TRY(tbn_launch_pack_stem_weight_rows(prm->weight + P->convs[0].w_off, wpack, 64, P->cin0, P->kw, P->stem_K, st));
  } else {
    TBN_TRY(tbn_launch_nchw_to_s2d_pad(x_nchw, ws + P->x0_off, R, P->cin0, P->H, P->W, st));
    TBN_TRY(tbn_launch_pack_stem_weight_s2d(prm->weight + P->convs[0].w_off, wpack, 64, P->cin0, st));
  }
  if (!training)
    TBN_TRY(tbn_launch_bn_fold(prm->gamma, prm->beta, prm->running_mean, prm->running_var, prm->bias, prm->eps, scale,
                               shift, (int)P->chan_floats, st));

  // TBN_BACKBONE_CONV_BF16X6 / _BF16X3 (eval forward only): every 3x3 / stride 1 / pad 1 layer on a map at most 64 wide goes
  // through the split-bf16 kernel as a single launch with the eval epilogue; its tile is the layer's tuned LDS-halo tile
  // where the plan holds one (same geometry), else that kernel's size heuristic.  The plan is not touched.
  const int bf16x_flag = training ? 0
                                  : ((prm->flags & TBN_BACKBONE_CONV_BF16X6) ? CONV_FLAG_BF16X6
                                                                             : ((prm->flags & TBN_BACKBONE_CONV_BF16X3) ? CONV_FLAG_BF16X3 : 0));
  auto bf16x_layer = [&](const Conv& c) {
    return bf16x_flag != 0 && conv_bf16x_layer(c) == BF16X_LAYER_3X3 && bf16x_3x3_map_ok(c.inW);
  };
  // TBN_BACKBONE_CONV_BF16X_ALL: those layers read their weight tiles from the caller's pre-split planes, and every
  // 1x1 / stride 1 GEMM (merged sibling groups with a pooled part included) goes through the pointwise split-bf16 kernel
  // with that kernel's size heuristic -- the plan holds no tile for it
  auto bf16x_pw_layer = [&](const Conv& c) { return bf16x_all && conv_bf16x_layer(c) == BF16X_LAYER_PW; };
  std::vector<long long> planes_off;
  if (bf16x_all) planes_layout(P, (bf16x_flag & CONV_FLAG_BF16X6) ? 6 : 3, &planes_off);
  const hipStream_t st_main = st;
  // riders: one-chain training program only; off while the profiler brackets the conv launches (a rider's time would be
  // charged to its host GEMM)
  const bool use_riders = training && !br && (prm->flags & TBN_BACKBONE_RIDERS) != 0 && !tbn_prof_enabled() && !P->riders.empty();
  RiderP pend_rider;        // a BN apply waiting for the conv launch that hosts it
  int pend_host = -1;
  if (training) PM->rider_launches[0] = 0;
  for (const Op& o : (br ? P->ops_b : P->ops)) {
    st = (br && o.side) ? side : st_main;   // the stream this op launches on
    if (o.kind == OP_FORK || o.kind == OP_JOIN) {
      sjoin.turn(PM->ev[ev_next++], o.kind == OP_FORK);
      continue;
    }
    if (o.kind == OP_CONV) {
      const Conv& c = P->convs[o.idx];
      const Conv::FwdTune& T = c.ft[tr];
      // a sibling pair with a split-bf16 member is issued as its two single launches (as branch mode does).  Eval only: the
      // training BN step reads pair_role as it is
      int role = pair_role(P, c, tr, br);
      if (role != 0 && (bf16x_layer(c) || bf16x_layer(P->convs[role == 1 ? c.pair_next : c.pair_prev]))) role = 0;
      if (role == 2) continue;   // ran with its sibling
      const RiderP* rd = (pend_host == o.idx) ? &pend_rider : nullptr;
      if (rd != nullptr) {
        pend_host = -1;
        ++PM->rider_launches[0];
      }
      ConvP p;
      if (role == 1) {
        const Conv& c2 = P->convs[c.pair_next];
        ConvP pb;
        for (int k = 0; k < 2; ++k) {   // both members keep their one-chain scratch slot (role 1 implies !br)
          const Conv& m = k ? c2 : c;
          fill_fwd(P, m, training, ws, prm->weight, R, k ? &pb : &p);
          fill_fwd_epilogue(P, m, training, ws, m.slot, k ? &pb : &p);
        }
        tbn_prof_label(("fwd " + c.parts[0].name + " | " + c2.parts[0].name).c_str());
        TBN_TRY(tbn_launch_conv_pair(p, pb, T.p_variant, T.p_mt, T.p_nt, st, rd));
        continue;
      }
      fill_fwd(P, c, training, ws, prm->weight, R, &p);
      fill_fwd_epilogue(P, c, training, ws, br ? c.slot_b : c.slot, &p);
      tbn_prof_label(("fwd " + c.parts[c.nparts - 1].name).c_str());
      const bool bx = bf16x_layer(c);
      if (bx || bf16x_pw_layer(c)) {
        p.flags |= bf16x_flag;
        p.halo = 0;
        if (bf16x_all) {
          p.flags |= CONV_FLAG_BF16X_PLANES;
          p.wt = reinterpret_cast<const float*>(static_cast<const char*>(prm->weight_planes) + planes_off[o.idx]);
        }
        const bool own_tile = bx && T.halo == 1;
        TBN_TRY(tbn_launch_conv(p, 0, own_tile ? T.mt : 0, own_tile ? T.nt : 0, st, nullptr));
        continue;
      }
      TBN_TRY(tbn_launch_conv(p, c.stem, T.mt, T.nt, st, rd));
    } else if (o.kind == OP_PREPOOL) {
      // pool_proj: 3x3 average of its conv output columns -> BN input (+ its batch statistics in training)
      const Conv& c = P->convs[o.idx];
      const Part& q = c.parts[o.part];
      const int M = R * c.outH * c.outW;
      const float* src = training ? ws + c.y_off + q.col0 : ws + q.yraw_off;
      const int src_ld = training ? c.cout : q.cout;
      if (!diag_skip(4)) TBN_TRY(tbn_launch_avgpool3_fwd(src, src_ld, ws + q.y2_off, q.cout, R, c.outH, c.outW, q.cout, 0, st));
      if (training) {
        int nparts = 0;
        TBN_TRY(tbn_launch_bn_stats(ws + q.y2_off, q.cout, M, q.cout,
                                    ws + P->partial_off + (size_t)(br ? q.slot_b : q.slot) * P->partial_floats, &nparts, st));
      }
    } else if (o.kind == OP_BN) {
      const BnStep& s = P->bns[o.idx];
      if (!training) {
        // only a pooled part still needs its (folded) BN + ReLU
        for (int k = 0; k < s.n; ++k) {
          const Conv& c = P->convs[s.conv[k]];
          const Part& q = c.parts[s.part[k]];
          if (!q.pooled) continue;
          const Buf& db = P->bufs[q.dst_buf];
          Seg z;
          z.ptr = ws + db.off + q.dst_choff;
          z.ld = db.C;
          z.col_begin = 0;
          if (!diag_skip(2))
            TBN_TRY(tbn_launch_bn_apply(ws + q.y2_off, R * c.outH * c.outW, q.cout, scale + q.c_off, shift + q.c_off, &z, 1, st));
        }
        continue;
      }
      const Conv& c0 = P->convs[s.conv[0]];
      if (s.n == 1 && c0.fuse_pool >= 0) {
        // conv -> BN -> ReLU -> max pool: the pool runs inside the BN apply (z is never written)
        const Part& q = c0.parts[0];
        const int M = R * c0.outH * c0.outW;
        const Pool& pl = P->pools[c0.fuse_pool];
        const Buf& ob = P->bufs[pl.outbuf];
        if (!diag_skip(2)) {
          TBN_TRY(tbn_launch_bn_finalize(ws + P->partial_off + (size_t)c0.slot * P->partial_floats, cdiv(M, writer_rows(P, c0, GEMM_FWD_TRAIN, br)), M,
                                         q.cout, prm->gamma + q.c_off, prm->beta + q.c_off, prm->bias + q.c_off,
                                         prm->running_mean + q.c_off, prm->running_var + q.c_off, prm->momentum, prm->eps,
                                         mean + q.c_off, rstd + q.c_off, scale + q.c_off, shift + q.c_off, st));
          TBN_TRY(tbn_launch_bn_apply_maxpool(ws + c0.y_off, (int)R, c0.outH, c0.outW, q.cout, scale + q.c_off,
                                              shift + q.c_off, ws + ob.off + pl.out_choff, ob.C,
                                              (uint8_t*)workspace + pl.argmax_off, ob.H, ob.W, pl.stride, pl.pad, st));
        }
        continue;
      }
      BnFwdBatch fb;
      memset(&fb, 0, sizeof(fb));
      fb.n = s.n;
      fb.momentum = prm->momentum;
      fb.eps = prm->eps;
      for (int k = 0; k < s.n; ++k) {
        const Conv& c = P->convs[s.conv[k]];
        const Part& q = c.parts[s.part[k]];
        const Buf& db = P->bufs[q.dst_buf];
        const int M = R * c.outH * c.outW;
        BnFwdLayer& L = fb.l[k];
        L.P = M;
        L.C = q.cout;
        if (q.pooled) {
          L.y = ws + q.y2_off;
          L.y_ld = q.cout;
          L.partial = ws + P->partial_off + (size_t)(br ? q.slot_b : q.slot) * P->partial_floats;
          L.pld = q.cout;
          L.nparts = tbn_bn_stats_parts(M, q.cout);
        } else {
          L.y = ws + c.y_off + q.col0;
          L.y_ld = c.cout;
          L.partial = ws + P->partial_off + (size_t)(br ? c.slot_b : c.slot) * P->partial_floats + q.col0;
          L.pld = c.cout;
          L.nparts = cdiv(M, writer_rows(P, c, GEMM_FWD_TRAIN, br));
        }
        L.gamma = prm->gamma + q.c_off;
        L.beta = prm->beta + q.c_off;
        L.conv_bias = prm->bias + q.c_off;
        L.running_mean = prm->running_mean + q.c_off;
        L.running_var = prm->running_var + q.c_off;
        L.save_mean = mean + q.c_off;
        L.save_rstd = rstd + q.c_off;
        L.scale = scale + q.c_off;
        L.shift = shift + q.c_off;
        L.nseg = 1;
        L.seg[0].ptr = ws + db.off + q.dst_choff;
        L.seg[0].ld = db.C;
        L.seg[0].col_begin = 0;
      }
      unsigned defer = 0;
      if (use_riders && P->bn_block[o.idx] >= 0) {
        const tbn_backbone_plan::BlockRiders& R = P->riders[P->bn_block[o.idx]];
        if (o.idx == R.bn_g && R.g_defer) {
          defer = R.g_defer;
          pend_host = R.c3;
        } else if (o.idx == R.bn_mid && R.mid_defer) {
          defer = R.mid_defer;
          pend_host = R.cd2;
        }
      }
      if (!diag_skip(2)) TBN_TRY(tbn_launch_bn_fwd_multi_defer(fb, defer, defer ? &pend_rider : nullptr, st));
    } else {
      const Pool& q = P->pools[o.idx];
      const Buf& ib = P->bufs[q.inbuf];
      const Buf& ob = P->bufs[q.outbuf];
      if (training && q.fused) continue;  // ran inside the producer's BN apply
      if (q.kind == 0) {
        if (!diag_skip(4)) TBN_TRY(tbn_launch_avgpool3_fwd(ws + ib.off, ib.C, ws + ob.off + q.out_choff, ob.C, R, ib.H, ib.W, ib.C, 0, st));
      } else {
        uint8_t* am = training ? (uint8_t*)workspace + q.argmax_off : nullptr;
        if (!diag_skip(4)) TBN_TRY(tbn_launch_maxpool_fwd(ws + ib.off, ib.C, ws + ob.off + q.out_choff, ob.C, am, R, ib.H, ib.W, ib.C,
                                       ob.H, ob.W, q.stride, q.pad, st));
      }
    }
  }
  st = st_main;   // (every block ends with a JOIN: the launch stream has seen all side-stream work)
  TBN_REQUIRE(pend_host < 0, "backbone_forward: a rider was left without its host launch (conv %d)", pend_host);
  *features_out = ws + P->bufs[P->out_buf].off;
  return TBN_OK;
}

}  // extern "C"

namespace {

// ---- autotune
constexpr int kMaxCand = 40;
struct Cand {
  int mt, nt, stages, halo;
  int variant;   // pair launches: tbn_launch_conv_pair's variant (0 LDS-halo members, 1 / 2 generic with 1 / 2 LDS stages)
};

// Experiment knobs (a -DTBN_EXPERIMENT=1 build only; the shipped library folds both to their defaults):
//   TBN_TUNE_MIN_TILE=n  candidates whose wave tile has fewer than n 32x32 sub-tiles are skipped where a larger tile
//                        exists (round-5 verdict item 1A: force the <1,1> class onto <1,2> / <2,1> / <2,2>)
//   TBN_TUNE_CORUN=k     every candidate is timed as k+1 concurrent copies (k helper streams beside the launch stream):
//                        what a launch costs in CU-time beside neighbours, not alone on an empty device.  The helper
//                        streams run the SAME candidate sequence in lockstep -- forked once in front of a GEMM's batch of
//                        candidates and joined once behind it: a fork / join per candidate (the first form of this knob)
//                        put ~70 us of cross-stream waits into every 50 - 150-us bracket and made the ranking noise
// What one autotune call owns on the device: a pair of timing events per candidate and the co-run helper streams.
struct TuneRig {
  hipEvent_t ce[2 * kMaxCand] = {};
  const int corun;
  hipStream_t hs[3] = {};
  hipEvent_t hfork = nullptr, hjoin[3] = {};
  bool ok = true;
  explicit TuneRig(int corun_) : corun(corun_) {
    for (hipEvent_t& e : ce) ok = ok && hipEventCreate(&e) == hipSuccess;
    for (int k = 0; k < corun; ++k) {
      (void)hipStreamCreateWithFlags(&hs[k], hipStreamNonBlocking);
      (void)hipEventCreateWithFlags(&hjoin[k], hipEventDisableTiming);
    }
    if (corun) (void)hipEventCreateWithFlags(&hfork, hipEventDisableTiming);
  }
  ~TuneRig() {
    for (hipEvent_t e : ce)
      if (e != nullptr) (void)hipEventDestroy(e);
    if (corun) {
      (void)hipDeviceSynchronize();
      (void)hipEventDestroy(hfork);
      for (int k = 0; k < corun; ++k) {
        (void)hipEventDestroy(hjoin[k]);
        (void)hipStreamDestroy(hs[k]);
      }
    }
  }
  TuneRig(const TuneRig&) = delete;
  TuneRig& operator=(const TuneRig&) = delete;
};

// Times the candidates of ONE GEMM (or sibling pair): `launch(cand, stream)` issues a candidate once.  All candidates are
// enqueued back to back, each as an untimed first run and a second run between its own pair of events, and the host waits
// ONCE (a host round trip per candidate cost more than the small layers' kernels themselves).  ms[k] = the measured time
// of candidate k.  The co-run copies (TBN_TUNE_CORUN): the same two launches, in the same order, on the helper streams --
// forked behind everything queued on `st`, joined behind the last candidate.
template <class Launch>
int time_candidates(TuneRig& X, hipStream_t st, const Cand* cand, int ncand, Launch&& launch, float* ms) {
  int rc = TBN_OK, timed = 0;
  if (X.corun) {
    (void)hipEventRecord(X.hfork, st);
    for (int h = 0; h < X.corun; ++h) (void)hipStreamWaitEvent(X.hs[h], X.hfork, 0);
  }
  for (int k = 0; k < ncand && rc == TBN_OK; ++k) {
    for (int h = 0; h < X.corun && rc == TBN_OK; ++h)
      for (int rep = 0; rep < 2 && rc == TBN_OK; ++rep) rc = launch(cand[k], X.hs[h]);
    if (rc == TBN_OK) rc = launch(cand[k], st);
    (void)hipEventRecord(X.ce[2 * k], st);
    if (rc == TBN_OK) rc = launch(cand[k], st);
    (void)hipEventRecord(X.ce[2 * k + 1], st);
    timed = k + 1;
  }
  for (int h = 0; h < X.corun; ++h) order_after(X.hjoin[h], X.hs[h], st);
  if (timed > 0) (void)hipEventSynchronize(X.ce[2 * timed - 1]);
  if (X.corun) (void)hipStreamSynchronize(st);
  for (int k = 0; k < ncand && rc == TBN_OK; ++k) {
    ms[k] = 0.f;
    (void)hipEventElapsedTime(&ms[k], X.ce[2 * k], X.ce[2 * k + 1]);
  }
  return rc;
}

// The fastest candidate (its index; -1: there is none).  A candidate is timed alone, back to back, on L2-warm operands; in
// the step its launches share the fabric with the HBM-bound BN kernels of the other streams.  The per-tap gather forms
// (register-staged / LDS-DMA) move 2-6x the bytes of the LDS-halo form on a 3x3 layer (profiles/r03_pmc_traffic.json):
// where an LDS-halo candidate exists, they must beat it by a margin to win.  The margin only RANKS: ms[] stays the time.
// (same-box A/B of the three-stream step: margin 0 -> 36.74, 6 % -> 36.49, 15 % -> 36.53 ms; one-stream GEMM totals equal.
//  A like margin AGAINST the single-stage register-staged loop -- more latency tolerance beside the other streams --
//  measured worse: 36.06 -> 36.33 / 36.38 ms at 5 / 12 %)
int rank_candidates(const Cand* cand, const float* ms, int ncand) {
  static const float halo_bias = 0.01f * (float)tbn_env_int("TBN_TUNE_HALO_BIAS", 8, 0, 100);
  bool any_halo = false;
  for (int k = 0; k < ncand; ++k) any_halo = any_halo || cand[k].halo == 1;
  float best = 1e30f;
  int bk = -1;
  for (int k = 0; k < ncand; ++k) {
    const float t = (any_halo && cand[k].halo != 1) ? ms[k] * (1.f + halo_bias) : ms[k];
    if (t < best) {
      best = t;
      bk = k;
    }
  }
  return bk;
}

}  // namespace

extern "C" {

// One-time tile autotuning: times every (MT, NT) tile of the forward and data-gradient implicit GEMM
// of each layer on the real shapes (2 launches each, hipEvents) and stores the fastest in the plan.
// Synchronises the device (the only entry point that does); activations in `workspace` are clobbered.
int tbn_backbone_autotune(tbn_backbone_plan* P, int training, const tbn_backbone_params* prm, void* workspace,
                          size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  TBN_REQUIRE(P && prm && workspace, "autotune: null argument");
  TBN_REQUIRE(workspace_bytes >= tbn_backbone_workspace_bytes(P, training), "autotune: workspace too small");
  float* ws = (float*)workspace;
  const int R = P->frames;
  const int tr = training ? 1 : 0;
  static const int min_tile = tbn_env_int("TBN_TUNE_MIN_TILE", 1, 1, 4);   // experiment knobs: see TuneRig
  static const int corun = tbn_env_int("TBN_TUNE_CORUN", 0, 0, 3);
  TuneRig rig(corun);
  if (!rig.ok) {
    tbn_set_error("autotune: hipEventCreate failed");
    return TBN_ERR_LAUNCH;
  }
  // candidates are timed one at a time: whatever other streams still run (the other modality backbones of a first
  // step) would make the choice depend on what happened to overlap -> drain the device first
  (void)hipDeviceSynchronize();
  Cand cand[kMaxCand];
  float ms[kMaxCand];
  for (auto& c : P->convs) {
    for (int pass = 0; pass < 2; ++pass) {  // 0: forward, 1: data gradient
      if (pass == 1 && (!training || !c.need_dgrad)) continue;
      if (pass == 0 && !training && c.nparts > 1) continue;   // eval tuning on single-part layers only keeps all writes in range
      const int rowmode = c.stem && pass == 0;
      ConvP p;
      if (pass == 0) {
        // the step's own epilogue, written into the layer's own y buffer (training) or its first destination (eval);
        // the statistics partials of every candidate go to scratch slot 0
        fill_fwd(P, c, training, ws, prm->weight, R, &p);
        fill_fwd_epilogue(P, c, training, ws, 0, &p);
        // the first destination only.  What the two calls leave anyway: training writes one y segment, and eval tunes
        // single-part layers, none of which is pooled (a pooled part, whose segment would be its raw buffer with
        // raw_seg1 set, only occurs as the last part of a fused 1x1 group of at least two parts)
        p.nseg = 1;
      } else {
        fill_dgrad(P, c, ws, R, &p);
      }
      // fastest of the candidates in isolation.  (Measured alternatives that lost: preferring the largest tile
      // within 3-15 % of the fastest -- monotonically slower steps; autotuning the weight-gradient tile the same
      // way -- 0.4 % slower than the size heuristic of tbn_wgrad_plan.)
      static const int force_halo = tbn_env_int("TBN_FORCE_HALO", -1, -1, 1);   // tests: 0 / 1
      static const int use_dma = tbn_env_int("TBN_USE_DMA", 1, 0, 1);
      static const int use_sk4 = tbn_env_int("TBN_USE_SK4", 1, 0, 1);
      int ncand = 0;
      for (int mt = 1; mt <= 2; ++mt)
        for (int nt = 1; nt <= 4; ++nt)
          for (int stg = 0; stg <= 4; ++stg) {                   // 0: LDS-halo kernel (3x3 / stride-1 layers), 3: LDS-DMA,
            if (32 * (nt - 1) >= p.Cout) continue;               // 4: 32-row tiles, waves split K (small maps)
            const int halo = stg == 0 ? 1 : (stg == 3 ? 2 : (stg == 4 ? 3 : 0));
            if (stg == 4) {
              if (rowmode || p.up != 1 || !use_sk4 || force_halo == 1 || p.M > kSk4MaxRows || mt > 2 || nt > 2) continue;
            } else if (stg == 3) {
              if (rowmode || p.up != 1 || !use_dma || force_halo == 1) continue;
            } else if (halo) {
              const size_t lb = rowmode ? 0 : tbn_conv_halo_lds_bytes(p, mt, nt);
              if (lb == 0 || lb > 160 * 1024 || force_halo == 0) continue;
            } else if (force_halo == 1 && !rowmode && tbn_conv_halo_lds_bytes(p, 1, 1) > 0) {
              continue;
            }
            if (ncand >= kMaxCand) continue;
            if (mt * nt < min_tile && (p.Cout > 32 || mt < 2) && !rowmode) continue;   // experiment: no small tiles
            cand[ncand++] = {mt, nt, stg == 3 ? 2 : (stg == 4 ? 1 : stg), halo, 0};
          }
      TBN_TRY(time_candidates(rig, st, cand, ncand, [&](const Cand& k, hipStream_t s) {
        p.halo = k.halo;
        p.stages = k.stages;
        return tbn_launch_conv(p, rowmode, k.mt, k.nt, s);
      }, ms));
      const int w = rank_candidates(cand, ms, ncand);
      const Cand win = w >= 0 ? cand[w] : Cand{1, 1, 2, 0, 0};
      const float t_win = w >= 0 ? ms[w] : 1e30f;
      if (pass == 0) {
        Conv::FwdTune& T = c.ft[tr];
        T.mt = win.mt;
        T.nt = win.nt;
        T.stages = win.stages;
        T.halo = win.halo;
        T.t = t_win;
      } else {
        c.d_mt = win.mt;
        c.d_nt = win.nt;
        c.d_stages = win.stages;
        c.d_halo = win.halo;
        c.t_dgrad = t_win;
      }
    }
  }
  // sibling pairs (3x3 | double_3x3_1): one launch for both when that beats the two tuned single launches
  static const int use_pairs = tbn_env_int("TBN_USE_PAIRS", 1, 0, 1);
  for (size_t ci = 0; ci < P->convs.size(); ++ci) {
    Conv& c = P->convs[ci];
    c.ft[tr].pair = false;
    if (training) c.pair_dgrad = false;      // an eval-mode tuning run leaves every data-gradient choice alone
    if (c.pair_next < 0 || !use_pairs) continue;
    Conv& c2 = P->convs[c.pair_next];
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 1 && (!training || c.stride != 1 || c2.stride != 1)) continue;   // stride 2: parity-phase launch
      ConvP pm[2];
      for (int k = 0; k < 2; ++k) {
        const Conv& m = k ? c2 : c;
        if (pass == 0) {   // as the single launches above, each member with its own scratch slot
          fill_fwd(P, m, training, ws, prm->weight, R, &pm[k]);
          fill_fwd_epilogue(P, m, training, ws, m.slot, &pm[k]);
          pm[k].nseg = 1;
        } else {
          fill_dgrad(P, m, ws, R, &pm[k]);
        }
      }
      int ncand = 0;
      for (int variant = 0; variant <= 2; ++variant) {
        if (variant == 0 && (tbn_conv_halo_lds_bytes(pm[0], 1, 1) == 0 || tbn_conv_halo_lds_bytes(pm[1], 1, 1) == 0)) continue;
        for (int mt = 1; mt <= 2; ++mt)
          for (int nt = 1; nt <= 2; ++nt) {
            if (variant == 0 && (tbn_conv_halo_lds_bytes(pm[0], mt, nt) > 160 * 1024 || tbn_conv_halo_lds_bytes(pm[1], mt, nt) > 160 * 1024))
              continue;
            if (ncand >= kMaxCand) continue;
            if (mt * nt < min_tile) continue;   // experiment: no small tiles (a (2, 1) pair tile always exists)
            cand[ncand++] = {mt, nt, variant == 2 ? 2 : 1, variant == 0 ? 1 : 0, variant};
          }
      }
      TBN_TRY(time_candidates(rig, st, cand, ncand, [&](const Cand& k, hipStream_t s) {
        return tbn_launch_conv_pair(pm[0], pm[1], k.variant, k.mt, k.nt, s);
      }, ms));
      const int w = rank_candidates(cand, ms, ncand);
      const Cand win = w >= 0 ? cand[w] : Cand{1, 1, 1, 0, 1};
      const float singles = pass == 0 ? c.ft[tr].t + c2.ft[tr].t : c.t_dgrad + c2.t_dgrad;
      // (margins of 0.88 / 1.05 instead of 0.97 measured 0.1-0.15 ms worse on the three-stream step; moving the weight flip
      //  to the tail of the forward, under the other streams, +-0: 36.81 vs 36.75 ms)
      const bool take = w >= 0 && ms[w] < 0.97f * singles;   // measured pair time against the measured singles
      if (pass == 0) {
        c.ft[tr].pair = take;
        c.ft[tr].p_variant = win.variant;
        c.ft[tr].p_mt = win.mt;
        c.ft[tr].p_nt = win.nt;
      } else {
        c.pair_dgrad = take;
        c.pd_variant = win.variant;
        c.pd_mt = win.mt;
        c.pd_nt = win.nt;
      }
    }
  }
  return TBN_OK;
}

int tbn_backbone_flip_weights(const tbn_backbone_plan* P, const tbn_backbone_params* prm, void* workspace, size_t workspace_bytes,
                              void* stream) {
  TBN_REQUIRE(P && prm && workspace && prm->weight, "backbone_flip_weights: null argument");
  TBN_REQUIRE(workspace_bytes >= P->total_bytes_train, "backbone_flip_weights: workspace too small (training workspace expected)");
  return tbn_launch_weight_flip_transpose_all(prm->weight, (float*)workspace + P->wt_off, P->flip, (hipStream_t)stream);
}

int tbn_backbone_backward(const tbn_backbone_plan* P, const float* dfeatures, const tbn_backbone_params* prm,
                          const tbn_backbone_grads* g, void* workspace, size_t workspace_bytes, void* stream) {
  TBN_REQUIRE(P && dfeatures && prm && g && workspace, "backbone_backward: null argument");
  TBN_REQUIRE(g->dweight && g->dbias, "backbone_backward: dweight/dbias required");
  TBN_REQUIRE(workspace_bytes >= P->total_bytes_train, "backbone_backward: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipStream_t aux = (hipStream_t)g->aux_stream;
  tbn_backbone_plan* PM = const_cast<tbn_backbone_plan*>(P);  // event pool only
  if (aux == st) aux = nullptr;
  constexpr int NE = tbn_backbone_plan::kEvents;
  // branch mode (see tbn_backbone_plan::ops_b): a side stream is given and nothing is being captured -- a captured
  // backward runs the serial program (a fork inside a capture is what the guard below is about)
  hipStream_t side = (hipStream_t)prm->side_stream;
  if (side == st || side == aux || P->ops_b.empty()) side = nullptr;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess) {
    (void)hipGetLastError();
    tbn_set_error("backbone_backward: hipStreamIsCapturing failed on the launch stream (invalid stream handle?)");
    return TBN_ERR_LAUNCH;
  }
  const bool capturing = cap != hipStreamCaptureStatusNone;
  if (capturing) side = nullptr;
  const bool br = side != nullptr;
  if ((aux != nullptr || br) && !capturing) TBN_TRY(ensure_events(PM));
  TBN_REQUIRE((aux == nullptr && !br) || capturing || (PM->n_ev == NE && (int)P->convs.size() + 2 * kNumBlocks + 3 + kGradBuckets < NE),
              "backbone_backward: event pool too small");
  if (aux != nullptr) {
    // Forking the weight-gradient stream from a stream that is itself a forked member of a capture (the modality streams
    // of a whole-step hipGraph) makes hipStreamEndCapture of ROCm 7.x (hip::Stream::EndCapture) recurse into itself until
    // the stack overflows -- a SIGSEGV after every call of the step has returned (profiles/r03_graph_capture_multi_aux_rocgdb.log).
    // Whether `st` is the capture's origin (a single-level fork captures fine) cannot be queried: refuse the combination.
    if (capturing) {
      tbn_set_error("backbone_backward: aux_stream inside a stream capture is not supported (nested capture forks overflow "
                    "the stack of hipStreamEndCapture in ROCm 7.x): capture with aux_stream = NULL");
      return TBN_ERR_UNSUPPORTED;
    }
  }
  // events 0..NE-2 fork (launch stream -> aux), the last one is the join: whatever path leaves this function, the aux
  // stream is joined back (a fork left open would also break hipGraph capture of a step)
  AuxJoin join{st, aux, aux != nullptr ? PM->ev[NE - 1] : nullptr};
  SideJoin sjoin{st, side, br ? PM->ev[NE - 2] : nullptr};   // (destroyed first: the side stream joins, then the aux stream)
  int ev_next = 0;
  float* ws = (float*)workspace;
  const int R = P->frames;
  float* mean = ws + P->stats_off;
  float* rstd = mean + P->chan_floats;
  float* scale = rstd + P->chan_floats;
  float* shift = scale + P->chan_floats;
  float* partial = ws + P->partial_off;
  float* coef = ws + P->coef_off;
  auto dptr = [&](int buf) -> const float* {
    return buf == P->out_buf ? dfeatures : ws + P->bufs[buf].doff;
  };

  if ((prm->flags & TBN_BACKBONE_WEIGHTS_FLIPPED) == 0)      // else: tbn_backbone_flip_weights ran on this workspace since the forward
    TBN_TRY(tbn_launch_weight_flip_transpose_all(prm->weight, ws + P->wt_off, P->flip, st));
  const std::vector<Op>& prog = br ? P->ops_b : P->ops;
  const hipStream_t st_main = st;
  const bool use_riders = !br && (prm->flags & TBN_BACKBONE_RIDERS) != 0 && !tbn_prof_enabled() && !P->riders.empty();
  RiderP bpend;             // BN-backward applies waiting for the data-gradient launch that hosts them
  int bpend_host = -1;
  PM->rider_launches[1] = 0;
  // branch mode without an aux stream: the weight gradients share ONE split-K slab region, so those of the side chain
  // are issued on the launch stream once the side chain has been joined
  int deferred[8], ndef = 0;
  const bool stem_last = !br && aux == nullptr && (prm->flags & TBN_BACKBONE_STEM_WGRAD_LAST) != 0;
  auto issue_wgrad = [&](const Conv& c, hipStream_t wst) -> int {
    tbn_prof_label(("wgrad " + c.parts[c.nparts - 1].name).c_str());
    WgradP wp;
    fill_wgrad(P, c, ws, R, &wp);
    if (c.stem) {
      float* dwp = ws + P->dwpack_off;
      TBN_TRY(tbn_launch_wgrad(wp, 1, dwp, ws + P->wsplit_off, wst));
      if (P->stem_mode == 1) return tbn_launch_unpack_stem_wgrad_rows(dwp, g->dweight + c.w_off, 64, P->cin0, P->kw, wst);
      return tbn_launch_unpack_stem_wgrad_s2d(dwp, g->dweight + c.w_off, 64, P->cin0, wst);
    }
    return tbn_launch_wgrad(wp, 0, g->dweight + c.w_off, ws + P->wsplit_off, wst);
  };
  // Gradient buckets (tbn_backbone_grads.bucket_cb): the walk runs from inception_5b down to the stem; once every op of
  // block 5a (then 4a) is enqueued, the weight gradients of that block and of all later ones are final in stream order --
  // a suffix of dweight the caller can start exchanging (RCCL all-reduce under data parallelism) while the 3x / stem
  // layers, the longest launches of a backward pass, are still to run.  Same points on every replica: the split depends on
  // the graph only.  Never inside a stream capture (the callback issues collectives).
  const int* blk_op = br ? P->block_op_b : P->block_op;
  size_t bucket_hi = P->weight_floats;
  auto fire_bucket = [&](int blk) -> int {
    const size_t lo = P->convs[P->block_conv[blk]].w_off;
    TBN_REQUIRE(ndef == 0, "backbone_backward: a weight gradient of block %d is still deferred at its bucket boundary", blk);
    if (aux != nullptr && join.forked) {   // the bucket's weight gradients ran on the aux stream: order the launch stream behind them
      order_after(PM->ev[ev_next++], aux, st_main);
    }
    g->bucket_cb(g->bucket_user, lo, bucket_hi - lo);
    bucket_hi = lo;
    return TBN_OK;
  };
  for (int oi = (int)prog.size() - 1; oi >= 0; --oi) {
    if (g->bucket_cb != nullptr && !capturing)
      for (int k = 0; k < kGradBuckets; ++k)
        if (oi + 1 == blk_op[kBucketBlock[k]]) TBN_TRY(fire_bucket(kBucketBlock[k]));
    const Op& o = prog[oi];
    st = (br && o.side) ? side : st_main;   // the stream this op launches on
    if (o.kind == OP_FORK || o.kind == OP_JOIN) {
      // reverse walk: a forward JOIN is where the side chain of the block STARTS (the block's output gradient is final),
      // a forward FORK where it is joined back, ahead of the 1x1 group's BN backward
      const bool fork = o.kind == OP_JOIN;
      sjoin.turn(PM->ev[ev_next++], fork);
      if (!fork) {
        for (int k = 0; k < ndef; ++k) TBN_TRY(issue_wgrad(P->convs[deferred[k]], st_main));
        ndef = 0;
      }
      continue;
    }
    if (o.kind == OP_POOL) {
      const Pool& q = P->pools[o.idx];
      const Buf& ib = P->bufs[q.inbuf];
      const Buf& ob = P->bufs[q.outbuf];
      if (q.inbuf == 0) continue;
      if (q.fused) continue;  // its gradient gather runs inside the producer's BN backward
      float* din = ws + ib.doff;
      if (q.kind == 0) {
        if (!diag_skip(4)) TBN_TRY(tbn_launch_avgpool3_fwd(dptr(q.outbuf) + q.out_choff, ob.C, din, ib.C, R, ib.H, ib.W, ib.C, q.bwd_accum,
                                        st));
      } else {
        if (!diag_skip(4)) TBN_TRY(tbn_launch_maxpool_bwd(dptr(q.outbuf) + q.out_choff, ob.C, (const uint8_t*)workspace + q.argmax_off,
                                       din, ib.C, R, ib.H, ib.W, ib.C, ob.H, ob.W, q.stride, q.pad, q.bwd_accum, st));
      }
      continue;
    }
    if (o.kind == OP_PREPOOL) {
      // the 3x3 average is self-adjoint: d(conv output columns) = avg_pool(d(pooled)), written next to the dy of the
      // other parts of the fused GEMM
      const Conv& c = P->convs[o.idx];
      const Part& q = c.parts[o.part];
      if (!diag_skip(4))
        TBN_TRY(tbn_launch_avgpool3_fwd(ws + q.y2_off, q.cout, ws + c.y_off + q.col0, c.cout, R, c.outH, c.outW, q.cout, 0, st));
      continue;
    }
    if (o.kind == OP_BN) {
      const BnStep& s = P->bns[o.idx];
      const Conv& c0 = P->convs[s.conv[0]];
      if (s.n == 1 && c0.fuse_pool >= 0) {
        const Part& q = c0.parts[0];
        const int M = R * c0.outH * c0.outW;
        const Pool& pl = P->pools[c0.fuse_pool];
        const Buf& ob = P->bufs[pl.outbuf];
        const float* dpool = dptr(pl.outbuf) + pl.out_choff;
        const uint8_t* am = (const uint8_t*)workspace + pl.argmax_off;
        float* y = ws + c0.y_off;
        const bool bn_grad = g->dgamma && g->dbeta && (g->bn_grad_layers == 2 || (g->bn_grad_layers == 1 && s.conv[0] == 0));
        if (!diag_skip(8)) {
          TBN_TRY(tbn_launch_bn_bwd_reduce_pooled(dpool, ob.C, am, R, c0.outH, c0.outW, ob.H, ob.W, pl.stride, pl.pad, y,
                                                  q.cout, scale + q.c_off, shift + q.c_off, mean + q.c_off,
                                                  rstd + q.c_off, partial, st));
          TBN_TRY(tbn_launch_bn_bwd_finalize(partial, tbn_bn_bwd_pooled_parts(R, c0.outH, c0.outW, q.cout, pl.stride, pl.pad), M,
                                             q.cout, scale + q.c_off,
                                             mean + q.c_off, rstd + q.c_off, coef, bn_grad ? g->dgamma + q.c_off : nullptr,
                                             bn_grad ? g->dbeta + q.c_off : nullptr, g->dbias + q.c_off, st));
          TBN_TRY(tbn_launch_bn_bwd_apply_pooled(dpool, ob.C, am, R, c0.outH, c0.outW, ob.H, ob.W, pl.stride, pl.pad, y,
                                                 q.cout, scale + q.c_off, shift + q.c_off, coef, y, st));
        }
        continue;
      }
      // one member of a batched BN-backward step: layer (conv ci, part pk) with the scratch slot `slot`
      auto fill_layer = [&](BnBwdLayer& L, int ci, int pk, int slot) {
        const Conv& c = P->convs[ci];
        const Part& q = c.parts[pk];
        const Buf& db = P->bufs[q.dst_buf];
        L.nseg = 1;
        L.dz[0].ptr = dptr(q.dst_buf) + q.dst_choff;
        L.dz[0].ld = db.C;
        L.dz[0].col_begin = 0;
        L.y = L.dy = q.pooled ? ws + q.y2_off : ws + c.y_off + q.col0;
        L.y_ld = q.pooled ? q.cout : c.cout;
        L.P = R * c.outH * c.outW;
        L.C = q.cout;
        L.scale = scale + q.c_off;
        L.shift = shift + q.c_off;
        L.mean = mean + q.c_off;
        L.rstd = rstd + q.c_off;
        if (q.red_src >= 0) {
          // S1 / S2 partials were formed by the data-gradient epilogue that finished dz (conv RedSeg)
          const Conv& f = P->convs[q.red_src];
          L.partial = ws + q.bpart_off;
          L.ext_parts = tbn_conv_red_rows(R, f.inH, f.inW, f.stride, f.k, f.pad, writer_rows(P, f, GEMM_DGRAD, br));
        } else {
          L.partial = partial + (size_t)slot * P->partial_floats;
          L.ext_parts = 0;
        }
        L.coef = coef + (size_t)slot * 3 * 1024;
        const bool first = (ci == 0);
        const bool bg = g->dgamma && g->dbeta && (g->bn_grad_layers == 2 || (g->bn_grad_layers == 1 && first));
        L.dgamma = bg ? g->dgamma + q.c_off : nullptr;
        L.dbeta = bg ? g->dbeta + q.c_off : nullptr;
        L.dbias = g->dbias + q.c_off;
      };
      BnBwdBatch bb;
      memset(&bb, 0, sizeof(bb));
      unsigned skip = 0, defer = 0;      // members another step already handled / members whose apply pass rides
      const tbn_backbone_plan::BlockRiders* RB = (use_riders && P->bn_block[o.idx] >= 0) ? &P->riders[P->bn_block[o.idx]] : nullptr;
      if (RB != nullptr && o.idx == RB->bn_g) skip = RB->g_defer;
      if (RB != nullptr && o.idx == RB->bn_mid) skip = RB->mid_defer;
      for (int k = 0; k < s.n; ++k)
        if (!(skip & (1u << k))) {
          fill_layer(bb.l[bb.n], s.conv[k], s.part[k], s.slot0 + bb.n);
          ++bb.n;
        }
      if (RB != nullptr && o.idx == RB->bn_d2 && (RB->g_defer | RB->mid_defer)) {
        // first BN step of the block in this (reverse) walk: the block's output gradient is final, so the members of the
        // LATER steps that write nothing the block's remaining GEMMs read -- `1x1`, `3x3`, `pool_proj` -- are reduced /
        // finalized here with double_3x3_2, and their apply pass rides in double_3x3_2's data-gradient launch
        for (int pass = 0; pass < 2; ++pass) {
          const BnStep& t = P->bns[pass == 0 ? RB->bn_g : RB->bn_mid];
          const unsigned m = pass == 0 ? RB->g_defer : RB->mid_defer;
          for (int k = 0; k < t.n; ++k)
            if (m & (1u << k)) {
              TBN_REQUIRE(bb.n < TBN_BN_MAXL, "backbone_backward: too many rider members");
              defer |= 1u << bb.n;
              fill_layer(bb.l[bb.n], t.conv[k], t.part[k], bb.n);
              ++bb.n;
            }
        }
        bpend_host = RB->cd2;
      }
      if (bb.n == 0) continue;      // every member rode in an earlier launch
      if (!diag_skip(8)) TBN_TRY(tbn_launch_bn_bwd_multi_defer(bb, defer, defer ? &bpend : nullptr, st));
      continue;
    }
    const Conv& c = P->convs[o.idx];
    // weight gradient -- on the aux stream when given: it only reads dy (final after the BN backward) and
    // the layer input, so it overlaps the data-gradient / BN-backward chain that continues on `st`
    if (aux != nullptr) {
      order_after(PM->ev[ev_next++], st, aux);
      join.forked = true;
      TBN_TRY(issue_wgrad(c, aux));
    } else if (br && o.side) {
      TBN_REQUIRE(ndef < 8, "backbone_backward: too many deferred weight gradients");
      deferred[ndef++] = o.idx;
    } else if (stem_last && (o.idx == 1 || o.idx == 2)) {
      // TBN_BACKBONE_STEM_WGRAD_LAST: the weight gradients of conv2_3x3 / conv2_3x3_reduce wait until conv1's pooled BN backward
      // (HBM-bound, 0.3 ms exposed when the three backward passes end together) is enqueued -- a GEMM of this stream then
      // runs while the other streams are in THEIR memory-bound tail.  Same kernels, same operands: bit-identical.
      deferred[ndef++] = o.idx;
    } else {
      TBN_TRY(issue_wgrad(c, st));
    }
    if (c.need_dgrad) {
      const int role = pair_role(P, c, GEMM_DGRAD, br);
      if (role == 2) continue;   // issued with its sibling (next in this walk)
      if (role == 1) {
        const Conv& c2 = P->convs[c.pair_next];
        ConvP pa, pb;
        fill_dgrad(P, c, ws, R, &pa);
        fill_dgrad(P, c2, ws, R, &pb);
        tbn_prof_label(("dgrad " + c.parts[0].name + " | " + c2.parts[0].name).c_str());
        TBN_TRY(tbn_launch_conv_pair(pa, pb, c.pd_variant, c.pd_mt, c.pd_nt, st));
        continue;
      }
      tbn_prof_label(("dgrad " + c.parts[c.nparts - 1].name).c_str());
      ConvP p;
      fill_dgrad(P, c, ws, R, &p);
      const RiderP* rd = (bpend_host == o.idx) ? &bpend : nullptr;
      if (rd != nullptr) {
        bpend_host = -1;
        ++PM->rider_launches[1];
      }
      TBN_TRY(tbn_launch_conv(p, 0, c.d_mt, c.d_nt, st, rd));
    }
  }
  if (stem_last) {
    for (int k = 0; k < ndef; ++k) TBN_TRY(issue_wgrad(P->convs[deferred[k]], st_main));
    ndef = 0;
  }
  TBN_REQUIRE(bpend_host < 0, "backbone_backward: a rider was left without its host launch (conv %d)", bpend_host);
  return TBN_OK;   // `join` joins the aux stream: everything the caller enqueues on `st` next sees the weight gradients
}

}  // extern "C"
