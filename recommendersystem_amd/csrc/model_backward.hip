// Backward pass of the trunk (autograd of transformer.model.py:493-529 restated): compact top, layers in reverse with the bucketed
// gradient hooks, grouped weight gradients, embedding / table gradients and the finalize stages.  Split from model.hip in round 5.
#include "model_internal.hpp"

namespace rsys {

// bf16 mode: the dx GEMMs of the trunk (dX = dY . W, W stored [out][in]) read W^T as a row-major [in][out] operand
static int ensure_transposes(Model* m) {
  if (!m->bf16_mode || !m->wt_dirty) return RSYS_OK;
  const int D = m->D, Ip = m->Ip;
  TransposeBatch b; b.n = 0;
  auto add = [&](int64_t off, int rows, int cols, long long ld) -> int {
    TransposeJob& j = b.job[b.n++];
    j.src = (const bf16*)m->Sh + off; j.dst = (bf16*)m->ShT + off; j.rows = rows; j.cols = cols; j.ld_src = ld; j.ld_dst = rows;
    if (b.n == 64) { int rc = launch_transpose_bf16(b, m->stream); b.n = 0; return rc; }
    return RSYS_OK;
  };
  for (int l = 0; l < m->L; ++l) {
    RC(add(m->lo[l].wqkv, m->Nqkv, D, D));
    RC(add(m->lo[l].wo, D, D, D));
    RC(add(m->lo[l].w13, 2 * Ip, D, D));
    RC(add(m->lo[l].w2, D, Ip, Ip));
  }
  RC(launch_transpose_bf16(b, m->stream));
  m->wt_dirty = false;
  return RSYS_OK;
}

// dX = dY . W for a trunk weight W [n_out][n_in] at offset `off`: bf16 mode reads the row-major transposed copy (ensure_transposes),
// the fp32 parity mode W itself, K-major
template <typename T>
static StepGemm gemm_dx(Model* m, const void* dY, int64_t off, int n_out, int n_in, void* dX, long long ldx, int M) {
  if (m->bf16_mode) return gemm_xwt(dY, n_out, WT<T>(m, off), n_out, dX, ldx, M, n_in, n_out);
  return gemm_dyw(dY, n_out, W<T>(m, off), n_in, dX, ldx, M, n_in, n_out);
}

// The rows the backward of a token-local tail runs on (model_forward.hip TailRows): what the forward kept of them, the gradient of the
// layer's output as fp32 residual (gx) and as GEMM operand (gxt), and where the gradients of the chain go.
struct TailGrads {
  int l, M;                         // layer; rows (compact: the buffers' capacity)
  const int* n_dev; int k_expect;   // compact: the device-side row count and the host's estimate of it; nullptr / 0: all M rows
  void *O, *hn, *ab, *g; float *h, *rstd2;
  void* gxt; float* gx;
  void *dab, *dhn; float* dh; void *dht, *dO;
  const char *tag_w2_dw, *tag_w2_dx, *tag_w13_dw, *tag_w13_dx, *tag_norm, *tag_o_dw, *tag_o_dx;   // (tag_norm == nullptr: not timed on its own)
  bool dense;                       // the dense rows' extras: the fp8 products, their weight gradients and f8_keep copies, reversed tile rows of W13's dx
};
static TailGrads tail_grads_dense(Model* m, int l, float* gx, void* gxt, void* dab, void* dht) {
  Model::LayerAct& a = m->la[l];
  return {l, 2 * m->cur_rows * m->S, nullptr, 0, a.O, a.hn, a.ab, a.g, a.h, a.rstd2, gxt, gx, dab, m->dhn, m->dh, dht, m->dO,
          "gemm_w2_dw", "gemm_w2_dx", "gemm_w13_dw", "gemm_w13_dx", "hbm_rmsnorm_bwd", "gemm_o_dw", "gemm_o_dx", true};
}
static TailGrads tail_grads_compact(Model* m) {
  return {m->L - 1, m->ctop_cap, m->c_n, expected_selected(m), m->c_O, m->c_hn, m->c_ab, m->c_g, m->c_h, m->c_rstd2, m->c_gx_t, m->c_gx,
          m->c_dab, m->c_dhn, m->c_dh, m->c_dh_t, m->c_dO,
          "gemm_top_w2_dw", "gemm_top_w2_dx", "gemm_top_w13_dw", "gemm_top_w13_dx", nullptr, "gemm_top_o_dw", "gemm_top_o_dx", false};
}

// Backward of layer_tail: W2 / SwiGLU / W13 / RMSNorm / Wo.  The weight gradients run in line here unless the base weights are frozen
// (finetune / adapter bank: only the dx chain runs, the LoRA tensors sit before the attention) or the dense rows' products are deferred
// to the grouped launch or run on the fp8 copies (behind the cast of their gradient operand, inside the dx product).  On compact rows they
// reduce over the device-side row count; each has one operand whose rows [n, n rounded up to 256) are zero.
template <typename T>
static int layer_tail_bwd(Model* m, const TailGrads& r, bool defer) {
  const int D = m->D, Ip = m->Ip, l = r.l;
  hipStream_t s = m->stream;
  const bool cp = m->bf16_mode;   // fp32 mode: the operand IS the fp32 buffer, no copy
  const bool f8 = r.dense && m->fp8, f8dw = r.dense && use_f8_dw(m);
  const bool dw = !trunk_frozen(m) && (!r.dense || (!defer && !f8dw));
  auto weight_grad = [&](const char* tag, const void* dY, long long ldy, const void* X, long long ldx, int64_t off, int M, int N) -> int {
    StepGemm p = gemm_dytx(dY, ldy, X, ldx, m->G + off, N, M, N, r.M);
    p.k_dev = r.n_dev; p.k_expect = r.k_expect;
    return gemm<T>(m, tag, p);
  };
  if (dw) RC(weight_grad(r.tag_w2_dw, r.gxt, D, r.g, Ip, m->lo[l].w2, D, Ip));   // dW2 += gx^T . g
  {
    StepGemm p = gemm_dx<T>(m, r.gxt, m->lo[l].w2, D, Ip, r.dab, 2 * Ip, r.M);   // dg = gx . W2, fused with the SwiGLU backward: writes [da|db] directly
    p.epi = EPI_SWIGLU_BWD; p.C2 = r.ab; p.ldc2 = 2 * Ip; p.m_dev = r.n_dev;
    if (f8) { p.f8_amax_out = f8_slot(m, l, F8S_DAB); RC(gemm_f8(m, l, F8P_W2_DX, r.tag_w2_dx, p, W8T(m, m->lo[l].w2), D, true)); }
    else RC(gemm<T>(m, r.tag_w2_dx, p));
    if (f8dw && !defer) RC(f8_dw_launch(m, l, 0, r.tag_w2_dw, r.M));
  }
  if (dw) RC(weight_grad(r.tag_w13_dw, r.dab, 2 * Ip, r.hn, D, m->lo[l].w13, 2 * Ip, D));   // dW13 += dab^T . hn
  {
    StepGemm p = gemm_dx<T>(m, r.dab, m->lo[l].w13, 2 * Ip, D, r.dhn, D, r.M);   // dhn = dab . W13
    p.m_dev = r.n_dev;
    // Tile rows from the LAST to the first, as the forward's W2 product (model_forward.hip layer_tail): this one reads dab behind w2_dx
    // (profiles/r6_ab_reverse_tile_rows.log: -2.4 % at this call site, nothing at the compact rows).
    if (r.dense && !f8) p.flags = GEMM_REVERSE_ROWS;
    if (f8) RC(gemm_f8(m, l, F8P_W13_DX, r.tag_w13_dx, p, W8T(m, m->lo[l].w13), 2 * Ip, true));   // (amax |da|, |db| came with the SwiGLU-backward epilogue)
    else RC(gemm<T>(m, r.tag_w13_dx, p));
    if (f8dw && !defer) RC(f8_dw_launch(m, l, 1, r.tag_w13_dw, r.M));
    if (r.dense && !m->f8_keep.empty()) HIP_CHECK(hipMemcpyAsync(m->f8_keep[l * 3 + 0], r.dhn, (size_t)r.M * D * 2, hipMemcpyDeviceToDevice, s));
  }
  if (r.tag_norm) tic(m, r.tag_norm, (sizeof(T) + 4.0 + 4.0 + 4.0 + (cp ? 2.0 : 0.0)) * D * r.M);   // g, x, residual gradient in; dx (+ its bf16 operand copy) out
  RC(launch_rmsnorm_bwd<T>(AT<T>(r.dhn), r.h, m->P + m->lo[l].mlp, r.rstd2, r.gx, r.dh, cp ? AT<T>(r.dht) : nullptr, small_grad(m, m->lo[l].mlp), r.M, D, s,
                           r.n_dev, nullptr, nullptr, f8 ? f8_slot(m, l, F8S_DH) : nullptr));
  if (r.tag_norm) toc(m);
  if (dw) RC(weight_grad(r.tag_o_dw, r.dht, D, r.O, D, m->lo[l].wo, D, D));   // dWo += dh^T . O
  {
    StepGemm p = gemm_dx<T>(m, r.dht, m->lo[l].wo, D, D, r.dO, D, r.M);   // dO = dh . Wo
    p.m_dev = r.n_dev;
    if (f8) RC(gemm_f8(m, l, F8P_O_DX, r.tag_o_dx, p, W8T(m, m->lo[l].wo), D, true));
    else RC(gemm<T>(m, r.tag_o_dx, p));
    if (f8dw && !defer) RC(f8_dw_launch(m, l, 2, r.tag_o_dw, r.M));
    if (r.dense && !m->f8_keep.empty()) HIP_CHECK(hipMemcpyAsync(m->f8_keep[l * 3 + 1], r.dO, (size_t)r.M * D * 2, hipMemcpyDeviceToDevice, s));
  }
  return RSYS_OK;
}

// That backward for the last layer's compact rows (gradients of all other tokens are identically zero there), then d(attention output)
// scattered into the dense buffer the attention backward reads.
template <typename T>
static int top_tail_compact_bwd(Model* m) {
  tic(m, "phase_top_compact_bwd");
  RC(layer_tail_bwd<T>(m, tail_grads_compact(m), false));
  // dO in selected-first order, as the attention backward reads it: the selected places from the compact rows, zeros up to the end of the last
  // query tile the kernels visit (c_qact); nothing is read beyond (round 6: was a 2 NT D-byte zero fill + a scatter)
  RC(launch_scatter_rows_fill<T>(AT<T>(m->c_dO), m->c_slot_p, m->c_qact, m->cur_rows, m->T, AT<T>(m->dO), m->D, m->D, m->stream));
  toc(m);
  return RSYS_OK;
}

// The four weight-gradient products of layers [l_lo, l_hi] from the operands the backward kept (Model::dwb), one grouped launch.
template <typename T>
static int grouped_weight_grads(Model* m, int l_lo, int l_hi) {
  const int D = m->D, Ip = m->Ip, NT = 2 * m->cur_rows * m->S;
  const bool top_compact = m->top_is_sparse;   // the last layer's W2 / W13 / Wo products ran on the compact rows already
  const bool f8 = use_f8_dw(m);                 // fp8 trunk: the products read the transposed fp8 copies instead
  const bool ordered = m->deterministic;        // the K splits' partial tiles to per-product slabs, added in index order
  const long long key = ((long long)ordered << 58) | ((long long)f8 << 57) | ((long long)top_compact << 56) | ((long long)l_lo << 40) | ((long long)l_hi << 32) | (unsigned int)m->cur_rows;
  auto it = m->dw_plans.find(key);
  if (it == m->dw_plans.end()) {
    std::vector<GemmParams> ps;
    for (int l = l_hi; l >= l_lo; --l) {
      const Model::LayerAct& a = m->la[l];
      const Model::DwOperands& o = m->dwb[l];
      auto add = [&](const void* A, long long lda, const void* B, long long ldb, float* C, long long ldc, int M, int N) {
        GemmParams p = gemm_dytx(A, lda, B, ldb, C, ldc, M, N, NT);
        p.alpha = 1.f;
        ps.push_back(p);
      };
      const bool full = !(top_compact && l == m->L - 1);
      if (f8) { for (int k : {1, 0, 3, 2}) ps.push_back(f8_dw_params(m, l, k, NT)); continue; }
      if (full) add(o.dab, 2 * Ip, a.hn, D, m->G + m->lo[l].w13, D, 2 * Ip, D);       // dW13 += dab^T . hn
      if (full) add(o.gxt, D, a.g, Ip, m->G + m->lo[l].w2, Ip, D, Ip);                 // dW2  += gx^T . g
      add(o.dqkv, m->Nqkv, a.xn, D, m->G + m->lo[l].wqkv, D, m->Nqkv, D);              // dWqkv += dqkv^T . xn
      if (full) add(o.dht, D, a.O, D, m->G + m->lo[l].wo, D, D, D);                    // dWo  += dh^T . O
    }
    GemmGroupPlan* pl = nullptr;
    ++m->host_stream_syncs;   // (first use of this layer range / batch size only)
    HIP_CHECK(hipStreamSynchronize(m->stream));
    if (m->dw_plans.size() >= 8) {   // (a plan bakes the row count in: a loader with many distinct last-batch sizes must not grow this without bound)
      for (auto& kv : m->dw_plans) gemm8p_group_plan_destroy(kv.second);
      m->dw_plans.clear();
    }
    RC(gemm8p_group_plan_create(ps.data(), (int)ps.size(), &pl, ordered));
    it = m->dw_plans.emplace(key, pl).first;
  }
  if (m->timer.enabled) tic(m, f8 ? "gemm_dw_group@8gf" : (gemm8p_group_on_4k(it->second) ? "gemm_dw_group@4kg" : "gemm_dw_group@8g"), gemm8p_group_flops(it->second));
  int rc = launch_gemm8p_group(it->second, m->stream);
  toc(m);
  if (rc == RSYS_OK && f8) rc = f8_dw_round_accum(m, l_lo, l_hi);
  return rc;
}

// ------------------------------------------------------------------ backward trunk + embeddings
template <typename T>
int backward_trunk(Model* m) {
  const int D = m->D, Ip = m->Ip, hd = m->hd, rows = m->cur_rows;
  const int N = rows * m->S, NT = 2 * N;
  hipStream_t s = m->stream;
  const int* rpos = m->resident.bd.rope_pos;
  float* gx = m->gxa;   // gradient w.r.t. the current layer's output (fp32 residual stream)
  float* gx_other = m->gxb;
  T* gxt = AT<T>(m->gxa_t);      // the same gradient as a GEMM operand (T)
  T* gxt_other = AT<T>(m->gxb_t);
  T* dht = AT<T>(m->dh_t);
  const bool cp = m->bf16_mode;  // fp32 mode: the operand IS the fp32 buffer, no copy
  // deferred weight gradients: the dY operands of layer l live in m->dwb[l] until the grouped launch that consumes them
  // (deterministic mode: the grouped launch in its ordered form -- bf16 products only, and the fp8 weight gradients are off in that mode)
  const bool det_group = sw().det_dw_group != 0;   // A/B: 0 = the per-layer slab path
  const bool defer = m->defer_dw && (!m->deterministic || (det_group && m->bf16_mode)) && !m->bank_train;   // (bank pass: no weight gradients at all)
  const bool ctop = m->top_is_sparse;
  if (defer && !ctop) gxt = AT<T>(m->dwb[m->L - 1].gxt);
  RC(ensure_transposes(m));
  tic(m, "phase_trunk_bwd");
  const double nb_bytes = (sizeof(T) + 4.0 + 4.0 + 4.0 + (cp ? 2.0 : 0.0)) * D * NT;   // g, x, residual gradient in; dx (+ its bf16 operand copy) out
  if (ctop) {   // final norm on the compact rows: c_gx = d(last layer's output) at the selected tokens, zero everywhere else
    RC(launch_rmsnorm_bwd_f32<T>(m->c_gy, m->c_xL, m->P + m->o_norm, m->c_rstdf, nullptr, m->c_gx, cp ? AT<T>(m->c_gx_t) : nullptr,
                                 small_grad(m, m->o_norm), m->ctop_cap, D, s, m->c_n));
  } else {
    tic(m, "hbm_rmsnorm_bwd", (4.0 + 4.0 + 4.0 + (cp ? 2.0 : 0.0)) * D * NT);
    RC(launch_rmsnorm_bwd_f32<T>(m->gy, m->xL, m->P + m->o_norm, m->rstdf, nullptr, gx, cp ? gxt : nullptr, small_grad(m, m->o_norm), NT, D, s, nullptr,
                                 m->fp8 ? f8_slot(m, m->L - 1, F8S_DY2) : nullptr));   // (fp8: the top layer's W2 takes this gradient as its dy)
    toc(m);
  }
  int bucket_top = m->L - 1;
  for (int l = m->L - 1; l >= 0; --l) {
    Model::LayerAct& a = m->la[l];
    const bool ft = trunk_frozen(m);        // finetune / adapter bank: base weights are frozen, only the dx chain and the LoRA grads run
    const bool own_lora = m->cfg.finetune != 0;   // the model's own adapter (the bank's gradients: adapter_bank_backward)
    const bool f8dw = use_f8_dw(m);         // fp8 weight gradients: launched behind the cast of their gradient operand (inside the dx product)
    const bool top = ctop && l == m->L - 1;   // this layer's token-local part runs on the compact rows
    void* const dab = (defer && !top) ? m->dwb[l].dab : m->dab;
    void* const dqkv = defer ? m->dwb[l].dqkv : m->dqkv;
    if (defer) { if (!top) dht = AT<T>(m->dwb[l].dht); gxt_other = l > 0 ? AT<T>(m->dwb[l - 1].gxt) : AT<T>(m->gxa_t); }
    if (top) RC(top_tail_compact_bwd<T>(m));
    else RC(layer_tail_bwd<T>(m, tail_grads_dense(m, l, gx, gxt, dab, dht), defer));
    // the last layer under the compact top: selected-first token order -- its ids, tile maps, RoPE positions; dO is non-zero in the leading query tiles only
    AttnParams ap = layer_attn<T>(m, l, top ? TOKENS_SELECTED_FIRST : TOKENS_BATCH);
    ap.rope_cos = m->rope_cos; ap.rope_sin = m->rope_sin; ap.rope_pos = top ? m->pos_p : rpos;
    if (top) ap.q_active = m->c_qact;
    ap.dO = m->dO; ap.delta = m->delta;
    ap.dq = dqkv; ap.dk = AT<T>(dqkv) + m->H * hd; ap.dv = AT<T>(dqkv) + (m->H + m->KV) * hd; ap.ldg = m->Nqkv;
    ap.f8_amax = m->fp8 ? f8_slot(m, l, F8S_DQKV) : nullptr;
    tic(m, "attn_bwd");
    RC(launch_attn_bwd<T>(ap, s));
    toc(m);
    if (!ft && !defer && !f8dw)   // dWqkv += dqkv^T . xn
      RC(gemm<T>(m, "gemm_qkv_dw", gemm_dytx(dqkv, m->Nqkv, a.xn, D, m->G + m->lo[l].wqkv, D, m->Nqkv, D, NT)));
    {
      StepGemm p = gemm_dx<T>(m, dqkv, m->lo[l].wqkv, m->Nqkv, D, m->dhn, D, NT);   // dxn = dqkv . Wqkv
      if (m->fp8) RC(gemm_f8(m, l, F8P_QKV_DX, "gemm_qkv_dx", p, W8T(m, m->lo[l].wqkv), m->Nqkv, true));
      else RC(gemm<T>(m, "gemm_qkv_dx", p));
      if (f8dw && !defer) RC(f8_dw_launch(m, l, 3, "gemm_qkv_dw", NT));
      if (!m->f8_keep.empty()) HIP_CHECK(hipMemcpyAsync(m->f8_keep[l * 3 + 2], m->dhn, (size_t)NT * D * 2, hipMemcpyDeviceToDevice, s));
    }
    if (m->bank_train) RC(adapter_bank_backward<T>(m, l, AT<T>(a.xn), AT<T>(dqkv), AT<T>(m->dhn)));
    if (own_lora) {
      T* xnd = m->drop_active ? AT<T>(a.xnd) : AT<T>(a.xn);
      const int nq = m->H * hd, nv0 = (m->H + m->KV) * hd, nkv = m->KV * hd;
      {
        StepGemm p = gemm_dyw(dqkv, m->Nqkv, W<T>(m, m->lo[l].lb), 16, m->dLa, 16, NT, 16, m->Nqkv);   // dLa = 2 * dqkv . Bcat    (the unused blocks of Bcat are zero)
        p.alpha = 2.f;
        RC(gemm<T>(m, "gemm_lora_dla", p));
      }
      {
        StepGemm p = gemm_dytx(dqkv, m->Nqkv, a.La, 16, m->G + m->lo[l].lb, 16, nq, 8, NT);   // dBq += 2 * dq^T . La[:, :8]
        p.alpha = 2.f;
        RC(gemm<T>(m, "gemm_lora_db", p));
      }
      {
        StepGemm p = gemm_dytx(AT<T>(dqkv) + nv0, m->Nqkv, AT<T>(a.La) + 8, 16, m->G + m->lo[l].lb + (int64_t)nv0 * 16 + 8, 16, nkv, 8, NT);   // dBv += 2 * dv^T . La[:, 8:]
        p.alpha = 2.f;
        RC(gemm<T>(m, "gemm_lora_db", p));
      }
      RC(gemm<T>(m, "gemm_lora_da", gemm_dytx(m->dLa, 16, xnd, D, m->G + m->lo[l].la, D, 16, D, NT)));   // d[Aq; Av] += dLa^T . drop(xn)
      {
        // dxn += dropout'(dLa . [Aq; Av])
        StepGemm p = gemm_dyw(m->dLa, 16, W<T>(m, m->lo[l].la), D, m->drop_active ? m->dxl : m->dhn, D, NT, D, 16);
        p.accum = m->drop_active ? 0 : 1;
        RC(gemm<T>(m, "gemm_lora_dx", p));
        if (m->drop_active)
          RC(launch_dropout<T>(AT<T>(m->dxl), AT<T>(m->dhn), (long long)NT * D, m->cfg.lora_dropout, m->drop_seed,
                               (unsigned int)(m->drop_step * 64 + l), 1, s));
      }
    }
    tic(m, "hbm_rmsnorm_bwd", nb_bytes);
    if (top)   // the residual gradient dh exists at the selected tokens only (compact rows, through the token -> row map)
      // ... and this layer's rows are in selected-first order: x is read at, and dx written to, the original token of each place
      RC(launch_rmsnorm_bwd<T>(AT<T>(m->dhn), a.x, m->P + m->lo[l].sa, a.rstd1, m->c_dh, gx_other, cp ? gxt_other : nullptr, small_grad(m, m->lo[l].sa), NT, D, s,
                               nullptr, m->c_slot_p, m->c_perm));
    else {
      RC(launch_rmsnorm_bwd<T>(AT<T>(m->dhn), a.x, m->P + m->lo[l].sa, a.rstd1, m->dh, gx_other, cp ? gxt_other : nullptr, small_grad(m, m->lo[l].sa), NT, D, s, nullptr, nullptr, nullptr,
                               (m->fp8 && l > 0) ? f8_slot(m, l - 1, F8S_DY2) : nullptr));   // (fp8: the layer below takes this gradient as its W2's dy)
    }
    toc(m);
    std::swap(gx, gx_other);
    std::swap(gxt, gxt_other);
    if (f8dw && !defer && !ft) RC(f8_dw_round_accum(m, l, l));   // (the layer's four products were launched one by one above)
    if (defer && !m->grad_bucket_hook && l == 0) RC(grouped_weight_grads<T>(m, 0, m->L - 1));   // all layers' products in one launch
    if (m->grad_bucket_hook && !ft) {
      // weight gradients of layers l .. bucket_top are final (the four tensors of a layer are contiguous, layers ascending)
      const int64_t lo = m->lo[l].wqkv, hi = m->lo[bucket_top].w2 + pad8((int64_t)D * Ip);
      // DDP's 25 MB buckets; with the grouped weight gradients a bucket is also a launch, and a grouped launch wants several
      // layers' products to fill the chip: two buckets (upper and lower half of the trunk) as long as each has its 25 MB
      const bool boundary = defer ? (l == m->L / 2 && (hi - lo) * 4 >= (25ll << 20)) : (hi - lo) * 4 >= (25ll << 20);
      if (l == 0 || boundary) {
        if (defer) RC(grouped_weight_grads<T>(m, l, bucket_top));   // the bucket's products, then its all-reduce
        RC(m->grad_bucket_hook(lo, hi));
        bucket_top = l - 1;
        // From here on all-reduce kernels share the CUs with the backward.  A persistent grid (one workgroup pinned per
        // CU, a fixed share of the tiles each) would stall on every CU a communication kernel holds, so the 256x256
        // GEMMs go back to one workgroup per tile until the reduction is over: the tiles flow to whatever CUs are free.
        m->gemm_flags |= GEMM_ONE_WG_PER_TILE;
      }
    }
  }
  toc(m);
  if (trunk_frozen(m)) return RSYS_OK;   // embeddings are frozen (model.py:361-369)
  // gx = gradient w.r.t. the interleaved input embeddings (even rows: items, odd rows: actions)
  tic(m, "phase_embed_bwd");
  BatchDev b = m->resident.bd; b.N = N; b.rows = rows; b.S = m->S;
  tic(m, "hbm_scatter", 12.0 * D * N);   // bytes: one gradient row read + one table-gradient row read-modify-written per interaction
  {
    const bool atomic_ab = sw().scatter_atomic != 0;   // A/B measurement against the float-atomic form only
    if (m->sharded) {
      // one gradient row per distinct id of the batch (keys = the ids' slots in the exchange plan, mask row = slot uV), sent
      // to the rows' owners; an owner adds what it receives requester by requester (the ids of one requester are distinct)
      HIP_CHECK(hipMemsetAsync(m->Frem, 0, (size_t)m->U * D * 4, s));
      RC(launch_embedding_scatter_segmented(gx, 2LL * D, b.m_matchedid, m->u_slot, m->tok_sidx, N, m->uV, D, m->Frem, m->scatter_slab, s));
      RC(comm_exchange(m->shard_comm, m->Frem, m->need_offD.data(), m->rows_xchg, m->serve_offD.data(), 4, s));
      for (int q = 0; q < m->sh_world; ++q) {
        const long long o = m->serve_off[q], n = m->serve_off[q + 1] - o;
        RC(launch_add_rows_by_id(m->rows_xchg + o * D, m->req_ids + o, m->row_lo, m->G + m->o_E, D, (int)n, D, s));
      }
    } else if (atomic_ab) RC(launch_embedding_scatter_add(gx, b, m->V, D, m->G + m->o_E, s));
    else {
      if (!m->tok_index_valid) {   // first backward over this batch: tokens sorted by (item id, position)
        RC(launch_token_index_build(b.matchedid, N, m->V, m->tok_keys, m->tok_skey, m->tok_sidx, s));
        m->tok_index_valid = true;
      }
      if (m->split_head_reduced) {
        // split table reduce: one row per distinct id of the batch in tok_T (the sharded path's compact scatter: keys = ranks of the
        // sorted ids, mask row = slot uV), added to G[E] from there -- the same sums in the same order as the direct scatter
        if (!m->split_plan_valid) {   // once per resident batch (one host sync: the launcher needs U and uV)
          RC(launch_plan_unique(m->tok_skey, m->tok_sidx, N, m->V, m->u_slot, m->u_ids, m->u_tok, m->u_plan, s));
          int plan[2];
          HIP_CHECK(hipMemcpyAsync(plan, m->u_plan, 8, hipMemcpyDeviceToHost, s));
          HIP_CHECK(hipStreamSynchronize(s));
          ARG_CHECK(plan[0] >= 1 && plan[0] <= N + 1 && plan[0] <= m->tok_cap && plan[1] >= 0 && plan[1] < plan[0], "split table reduce: inconsistent list of distinct ids");
          m->U = plan[0]; m->uV = plan[1];
          m->split_plan_valid = true;
        }
        HIP_CHECK(hipMemsetAsync(m->tok_T, 0, (size_t)m->U * D * 4, s));
        RC(launch_embedding_scatter_segmented(gx, 2LL * D, b.m_matchedid, m->u_slot, m->tok_sidx, N, m->uV, D, m->tok_T, m->scatter_slab, s));
        // G[E] is still the SEND buffer of the head part's out-of-place all-reduce on the communicator's stream (capi.hip
        // table_head_hook): the first write to it since then waits for that collective to have read it
        if (m->split_head_event) HIP_CHECK(hipStreamWaitEvent(s, m->split_head_event, 0));
        RC(launch_add_rows_by_id(m->tok_T, m->u_ids, 0, m->G + m->o_E, D, m->U, D, s));
      } else
      RC(launch_embedding_scatter_segmented(gx, 2LL * D, b.m_matchedid, m->tok_skey, m->tok_sidx, N, m->V, D, m->G + m->o_E, m->scatter_slab, s));
    }
  }
  toc(m);
  m->table_grads_pending = true;
  m->gE_clean[0] = m->gE_clean[1] = false;   // the rows now hold token gradients: a later head GEMM must add, not store
  RC(gemm<T>(m, "gemm_action_dw", gemm_dytx(gxt + D, 2 * D, m->feat, 32, m->G + m->o_lin_w, 32, D, 32, N)));   // dWlin += g_act^T . feat
  RC(launch_colsum_add(gx + D, 2 * D, N, D, m->G + m->o_lin_b, s));
  {
    StepGemm p = gemm_dyw(gxt + D, 2 * D, W<T>(m, m->o_lin_w), 32, m->gf, 32, N, 32, D);   // gf = g_act . Wlin
    p.c_f32 = 1;
    RC(gemm<T>(m, "gemm_action_dx", p));
  }
  SmallParams sp = small_params(m);
  RC(launch_action_small_bwd(m->gf, b, sp, m->G + m->o_pcos, m->G + m->o_psin, m->G + m->o_status, m->G + m->o_gender,
                             m->G + m->o_source, s));
  toc(m);
  return RSYS_OK;
}

// dWp = dF^T Meta and dbp = colsum(dF), once per optimizer step from the accumulated dF (= grad of E).
// stage 1: operand copy of dF + bias gradient (afterwards nothing reads G[E] any more: in bf16 mode the GEMM works on the
// copy, so the gradient all-reduce of the item table can run beside it); stage 2: the GEMM; stage 0: both.
template <typename T>
static int finalize_grads_t(Model* m, int stage) {
  tic(m, stage == 2 ? "phase_table_bwd_gemm" : "phase_table_bwd");
  const bool direct = m->bf16_mode && m->D % 64 == 0;   // fp32 dF -> bf16 dF^T + bias gradient in one pass
  if (stage != 2 && direct) {
    RC(launch_cast_transpose_colsum(m->G + m->o_E, (bf16*)m->dFT, m->TR, m->D, m->Vp, m->G + m->o_bp, m->stream));
  } else if (stage != 2) {
    m->table_dirty = true;   // (FT is borrowed below)
    const bool fused = m->bf16_mode && m->D <= 1024 && 1024 % (m->D >> 2) == 0;
    if (fused) {   // operand copy of dF in the fused-table buffer (dead until the next forward rebuilds it) + bias gradient, one pass
      RC(launch_cast_colsum(m->G + m->o_E, (bf16*)m->FT, m->TR, m->D, m->G + m->o_bp, m->stream));
    } else {
      if (m->bf16_mode) RC(launch_cast<bf16>(m->G + m->o_E, (bf16*)m->FT, (long long)m->TR * m->D, m->stream));
      RC(launch_colsum_add(m->G + m->o_E, m->D, m->TR, m->D, m->G + m->o_bp, m->stream));
    }
    if (m->bf16_mode) {   // K-contiguous copy of dF for the row-major pipeline: dFT[d][v]
      TransposeBatch b; b.n = 1;
      b.job[0].src = (const bf16*)m->FT; b.job[0].dst = (bf16*)m->dFT; b.job[0].rows = m->TR; b.job[0].cols = m->D;
      b.job[0].ld_src = m->D; b.job[0].ld_dst = m->Vp;
      RC(launch_transpose_bf16(b, m->stream));
    }
  }
  if (stage != 1) {
    float* dWp = m->G + m->o_Wp;
    if (m->bf16_mode) {   // dWp[d][c] += sum_v dFT[d][v] MetaT[c][v]  (both operands K-contiguous, padding columns are zero)
      StepGemm p = gemm_xwt(m->dFT, m->Vp, m->MetaT, m->Vp, dWp, m->Mp, m->D, m->Mp, (int)m->Vp);
      p.c_f32 = 1; p.epi = EPI_ATOMIC;
      RC(gemm<T>(m, "gemm_table_dw", p));
    } else {
      RC(gemm<T>(m, "gemm_table_dw", gemm_dytx(m->G + m->o_E, m->D, m->Meta, m->Mp, dWp, m->Mp, m->D, m->Mp, m->TR)));
    }
  }
  toc(m);
  return RSYS_OK;
}

int model_finalize_grads(Model* m) {
  if (!m->table_grads_pending || m->cfg.finetune) return RSYS_OK;
  DetScope det(m);
  m->table_grads_pending = false;
  return m->bf16_mode ? finalize_grads_t<bf16>(m, 0) : finalize_grads_t<float>(m, 0);
}

// the two halves separately (gradient all-reduce overlap, capi.hip); only when model_finalize_splittable
bool model_finalize_splittable(const Model* m) { return m->table_grads_pending && !m->cfg.finetune && m->bf16_mode; }

// ---- split reduce of the replicated item table's gradient (model.hpp; armed per backward by rsys_set_grad_sync)
int model_split_table_enable(Model* m, int on) {
  if (!on) { m->split_table = false; m->table_head_hook = nullptr; return RSYS_OK; }
  ARG_CHECK(!m->sharded, "split table reduce: the item table is row-sharded (its rows are reduced by their owners already)");
  ARG_CHECK(m->bf16_mode && !m->cfg.finetune, "split table reduce: bf16 training of the full model only (the fp32 mode's metadata-projection gradient reads G[E] itself)");
  HIP_CHECK(hipSetDevice(m->device));
  if (!m->tbl_R) {
    const int64_t N = (int64_t)m->rows_max * m->Sa;
    m->tok_cap = N + 1;
    DALLOC(m->tbl_R, (int64_t)m->TR * m->D * 4);
    DALLOC(m->tok_T, m->tok_cap * m->D * 4);
    if (!m->u_slot) { DALLOC(m->u_slot, N * 4); DALLOC(m->u_ids, (N + 1) * 4); DALLOC(m->u_tok, N * 4); DALLOC(m->u_plan, 64); }
  }
  m->split_table = true;
  return RSYS_OK;
}

// rows per rank the tail's all-gathers carry: the maximum over the ranks of the batches' distinct-id bounds (model_split_table_arm formed it
// at the head of the communicator's stream a whole backward ago), at least this rank's exact U, at most the lists' capacity
int model_split_table_rows(Model* m, int64_t* rows) {
  int64_t n = m->tok_cap;
  if (m->umax_pending) {
    HIP_CHECK(hipEventSynchronize(m->ev_umax));
    m->umax_pending = false;
    const int64_t got = (int64_t)m->h_umax[1];
    ARG_CHECK(got >= m->U && got <= m->tok_cap, "split table reduce: the ranks' maximum of distinct ids is smaller than this rank's own list");
    n = (got + 63) / 64 * 64;          // (whole 256-byte id blocks per rank)
    if (n > m->tok_cap) n = m->tok_cap;
  }
  *rows = n;
  return RSYS_OK;
}
int model_split_table_arm(Model* m, rsys_comm* c) {
  if (m->h_umax == nullptr) {
    HIP_CHECK(hipHostMalloc((void**)&m->h_umax, 64, hipHostMallocDefault));
    HIP_CHECK(hipMalloc((void**)&m->d_umax, 64));
    HIP_CHECK(hipEventCreateWithFlags(&m->ev_umax, hipEventDisableTiming));
  }
  // (a batch staged before the split reduce was switched on has no count: the lists' capacity then)
  const int64_t bound = (m->u_bound_host >= 1 && m->u_bound_host <= m->tok_cap) ? m->u_bound_host : m->tok_cap;
  if (m->umax_pending) HIP_CHECK(hipEventSynchronize(m->ev_umax));   // (an armed step that never reached its tail)
  m->h_umax[0] = (float)bound;                                         // (< 2^24: exact)
  HIP_CHECK(hipMemcpyAsync(m->d_umax, m->h_umax, 4, hipMemcpyHostToDevice, c->stream));
  RC(comm_all_reduce_f32(c, m->d_umax, 1, COMM_MAX, c->stream));
  HIP_CHECK(hipMemcpyAsync(m->h_umax + 1, m->d_umax, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_CHECK(hipEventRecord(m->ev_umax, c->stream));
  m->umax_pending = true;
  return RSYS_OK;
}

int model_split_table_tail(Model* m, rsys_comm* c, hipStream_t cs, int64_t* rows_out) {
  const int W = comm_active(c) ? c->world : 1, D = m->D;
  int64_t cap = 0;
  RC(model_split_table_rows(m, &cap));
  if (rows_out) *rows_out = cap;
  if (m->tok_all_world < W || m->tok_all_rows < cap) {
    for (void* p : {(void*)m->tok_Tall, (void*)m->tok_Uall, (void*)m->tok_Pall}) if (p) HIP_CHECK(hipFree(p));
    m->tok_Tall = nullptr; m->tok_Uall = nullptr; m->tok_Pall = nullptr;
    const int64_t rows = std::min<int64_t>(m->tok_cap, cap + cap / 8);   // (some room: the next batches' maxima differ by a few percent)
    HIP_CHECK(hipMalloc((void**)&m->tok_Tall, (size_t)W * rows * D * 4));
    HIP_CHECK(hipMalloc((void**)&m->tok_Uall, (size_t)W * rows * 4));
    HIP_CHECK(hipMalloc((void**)&m->tok_Pall, (size_t)W * 64));
    m->tok_all_world = W; m->tok_all_rows = rows;
  }
  // rows [U_r, cap) of a rank's list hold whatever an earlier batch left there: they travel, nobody adds them (the counted add stops at the
  // rank's own U from its gathered plan)
  RC(comm_all_gather(c, m->tok_T, m->tok_Tall, (size_t)cap * D * 4, cs));
  RC(comm_all_gather(c, m->u_ids, m->tok_Uall, (size_t)cap * 4, cs));
  RC(comm_all_gather(c, m->u_plan, m->tok_Pall, 64, cs));
  HIP_CHECK(hipMemcpyAsync(m->G + m->o_E, m->tbl_R, (size_t)m->TR * D * 4, hipMemcpyDeviceToDevice, cs));
  for (int q = 0; q < W; ++q)   // rank order: every rank adds the same rows in the same order
    RC(launch_add_rows_by_id_counted(m->tok_Tall + (size_t)q * cap * D, m->tok_Uall + (size_t)q * cap, m->tok_Pall + (size_t)q * 16,
                                     m->G + m->o_E, D, (int)cap, D, cs));
  return RSYS_OK;
}
int model_finalize_stage(Model* m, int stage, int64_t* wp_off, int64_t* wp_n) {
  if (wp_off) *wp_off = m->o_Wp;
  if (wp_n) *wp_n = (int64_t)m->D * m->Mp;
  if (stage == 2) m->table_grads_pending = false;
  DetScope det(m);
  return finalize_grads_t<bf16>(m, stage);
}

template int backward_trunk<float>(Model*);
template int backward_trunk<bf16>(Model*);

}  // namespace rsys
