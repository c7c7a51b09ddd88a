// Python bindings for the kubeai_amd gfx950 HIP kernels.
#include <torch/extension.h>

#include <tuple>
#include <utility>

#include "attention_plan.h"

void rmsnorm(torch::Tensor out, torch::Tensor x, torch::Tensor weight,
             double eps);
void fused_add_rmsnorm(torch::Tensor x, torch::Tensor residual,
                       torch::Tensor weight, double eps);
void rope(torch::Tensor q, torch::Tensor k, torch::Tensor positions,
          torch::Tensor cos_sin);
void rope_and_cache(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                    torch::Tensor positions, torch::Tensor cos_sin,
                    torch::Tensor k_cache, torch::Tensor v_cache,
                    torch::Tensor slot_mapping);
void reshape_and_cache(torch::Tensor k, torch::Tensor v, torch::Tensor k_cache,
                       torch::Tensor v_cache, torch::Tensor slot_mapping);
void paged_attention_decode(torch::Tensor out, torch::Tensor q,
                            torch::Tensor k_cache, torch::Tensor v_cache,
                            torch::Tensor block_tables, torch::Tensor seq_lens,
                            double scale, int64_t window, double softcap);
void paged_attention_decode_fp8(torch::Tensor out, torch::Tensor out_fp8,
                                torch::Tensor out_scale, torch::Tensor q,
                                torch::Tensor k_cache, torch::Tensor v_cache,
                                torch::Tensor block_tables,
                                torch::Tensor seq_lens, double scale,
                                int64_t window, double softcap);
void rope_cache_attention_decode(
    torch::Tensor out, c10::optional<torch::Tensor> out_fp8,
    c10::optional<torch::Tensor> out_scale, torch::Tensor q, torch::Tensor k,
    torch::Tensor v, torch::Tensor positions, torch::Tensor cos_sin,
    torch::Tensor k_cache, torch::Tensor v_cache, torch::Tensor slot_mapping,
    torch::Tensor block_tables, torch::Tensor seq_lens, double scale,
    int64_t window, double softcap);
void paged_attention_prefill(torch::Tensor out, torch::Tensor q,
                             torch::Tensor k_cache, torch::Tensor v_cache,
                             torch::Tensor block_tables,
                             torch::Tensor query_start_loc,
                             torch::Tensor seq_lens, double scale,
                             int64_t window, double softcap);
void silu_and_mul(torch::Tensor out, torch::Tensor x);
void gelu_and_mul(torch::Tensor out, torch::Tensor x);
void skinny_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor w);
// W4A16 (int4_gemm.hip); (qp, sp, zp) is Int4Weight's packed layout
void int4_dequant(torch::Tensor out, torch::Tensor qp, torch::Tensor sp,
                  torch::Tensor zp, int64_t N, int64_t K, int64_t group);
void int4_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor qp,
               torch::Tensor sp, torch::Tensor zp, int64_t N, int64_t K,
               int64_t group);
int64_t int4_gemm_tiles(int64_t N, int64_t M);
// grouped MoE expert GEMMs routed on the device (int4_moe.hip); table is the
// int64 [E, 3] of the experts' (qp, sp, zp) addresses
void int4_moe_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor selected,
                   torch::Tensor table, int64_t row_div, int64_t E, int64_t N,
                   int64_t K, int64_t group, int64_t n_tiles);
void moe_combine(torch::Tensor out, torch::Tensor y, torch::Tensor selected,
                 torch::Tensor weights, int64_t E);
std::tuple<int64_t, int64_t> int4_moe_plan(int64_t N, int64_t T, int64_t E,
                                           int64_t k);
// the fp8 sibling (fp8_moe.hip); table is the int64 [E, 2] of the experts'
// (weight_fp8, weight_scale) addresses
void fp8_moe_gemm(torch::Tensor y, torch::Tensor xq, torch::Tensor xs,
                  torch::Tensor selected, torch::Tensor table, int64_t row_div,
                  int64_t E, int64_t N, int64_t K, int64_t n_tiles);
std::tuple<int64_t, int64_t> fp8_moe_plan(int64_t N, int64_t T, int64_t E,
                                          int64_t k);
void greedy_sample(torch::Tensor out, torch::Tensor logits);
void gumbel_sample(torch::Tensor out, torch::Tensor logits,
                   torch::Tensor temperature, torch::Tensor seeds,
                   int64_t step);
void greedy_sample_logprob(torch::Tensor out, torch::Tensor out_logprob,
                           torch::Tensor out_lse, torch::Tensor logits);
void gumbel_sample_logprob(torch::Tensor out, torch::Tensor out_logprob,
                           torch::Tensor out_lse, torch::Tensor logits,
                           torch::Tensor temperature, torch::Tensor seeds,
                           int64_t step);
void token_logprobs(torch::Tensor out_logprob, torch::Tensor out_lse,
                    torch::Tensor logits, torch::Tensor tokens);
void sgmv(torch::Tensor y, torch::Tensor x, torch::Tensor A, torch::Tensor B,
          torch::Tensor idx, double scale);
void register_chwbl(pybind11::module_& m);
// one-shot fused all-reduce over xGMI (allreduce.hip)
pybind11::bytes xgmi_alloc();
void xgmi_connect(int64_t rank, int64_t world,
                  const std::vector<pybind11::bytes>& handles);
void xgmi_fused_allreduce_add_rmsnorm(torch::Tensor x, torch::Tensor residual,
                                      torch::Tensor weight, double eps);
int64_t xgmi_error_count();
int64_t xgmi_max_elems();
void xgmi_shutdown();
void rmsnorm_fp8(torch::Tensor out, torch::Tensor out_scale, torch::Tensor x,
                 torch::Tensor weight, double eps);
void fused_add_rmsnorm_fp8(torch::Tensor out, torch::Tensor out_scale,
                           torch::Tensor x, torch::Tensor residual,
                           torch::Tensor weight, double eps);
void fused_add_rmsnorm_fp8_div(torch::Tensor out, torch::Tensor out_scale,
                               torch::Tensor x, torch::Tensor residual,
                               torch::Tensor weight, double eps,
                               bool write_rows);
void embed_rmsnorm_fp8(torch::Tensor out, torch::Tensor out_scale,
                       torch::Tensor x_out, torch::Tensor ids,
                       torch::Tensor table, torch::Tensor weight, double eps);
void silu_and_mul_fp8(torch::Tensor out, torch::Tensor out_scale,
                      torch::Tensor x);
void quant_fp8(torch::Tensor out, torch::Tensor out_scale, torch::Tensor x);
void quant_fp8_div(torch::Tensor out, torch::Tensor out_scale,
                   torch::Tensor x);
void nucleus_stats(torch::Tensor m, torch::Tensor z, torch::Tensor logits,
                   torch::Tensor temps);
void nucleus_accept(torch::Tensor ok, torch::Tensor logits,
                    torch::Tensor cand, torch::Tensor m, torch::Tensor z,
                    torch::Tensor temps, torch::Tensor top_ps,
                    torch::Tensor top_ks);

// the launch plans the attention launchers follow (attention_plan.h)
static std::pair<int64_t, int64_t> prefill_plan(int64_t Tq, int64_t B,
                                                int64_t n_q, int64_t n_kv,
                                                int64_t hd, int64_t max_blocks,
                                                int64_t window,
                                                double softcap) {
  TORCH_CHECK(n_kv > 0 && n_q % n_kv == 0);
  const attn_plan::PrefillPlan p = attn_plan::prefill_plan(
      Tq, (int)B, (int)n_q, (int)n_kv, (int)hd, (int)max_blocks, window,
      softcap);
  return {p.version, p.waves};
}
static int64_t decode_plan(int64_t B, int64_t n_kv, int64_t max_blocks) {
  return attn_plan::decode_n_splits((int)B, (int)n_kv, (int)max_blocks);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("prefill_plan", &prefill_plan,
        "(version, waves per workgroup) paged_attention_prefill launches",
        pybind11::arg("Tq"), pybind11::arg("B"), pybind11::arg("n_q"),
        pybind11::arg("n_kv"), pybind11::arg("hd"),
        pybind11::arg("max_blocks"), pybind11::arg("window") = 0,
        pybind11::arg("softcap") = 0.0);
  m.def("decode_plan", &decode_plan,
        "flash-decoding splits paged_attention_decode launches",
        pybind11::arg("B"), pybind11::arg("n_kv"),
        pybind11::arg("max_blocks"));
  m.def("rmsnorm", &rmsnorm, "RMSNorm (bf16, fp32 accum)");
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm,
        "in-place residual add + RMSNorm");
  m.def("rope", &rope, "NeoX rotary embedding, in-place q/k");
  m.def("rope_and_cache", &rope_and_cache,
        "rotary embedding (in-place q/k) fused with the paged KV cache write");
  m.def("reshape_and_cache", &reshape_and_cache,
        "paged KV cache write (bf16 or fp8 e5m2 cache)");
  m.def("paged_attention_decode", &paged_attention_decode,
        "paged attention, one query token per seq");
  m.def("paged_attention_decode_fp8", &paged_attention_decode_fp8,
        "paged decode attention that also emits the e4m3 row quant of out");
  m.def("rope_cache_attention_decode", &rope_cache_attention_decode,
        "pure-decode step: rotary embedding and KV cache write inside the "
        "decode attention kernel (q, k, v are only read)");
  m.def("paged_attention_prefill", &paged_attention_prefill,
        "paged causal flash attention over cached KV");
  m.def("gelu_and_mul", &gelu_and_mul, "GeGLU tanh-gelu(gate)*up");
  m.def("silu_and_mul", &silu_and_mul, "SwiGLU activation");
  m.def("skinny_gemm", &skinny_gemm, "weight-streaming GEMM for M<=64");
  m.def("int4_dequant", &int4_dequant,
        "packed int4 weight -> bf16 [N, K], bit-equal to Int4Weight.dequant()");
  m.def("int4_gemm", &int4_gemm,
        "fused dequant + GEMM over a packed int4 weight, M <= 64");
  m.def("int4_gemm_tiles", &int4_gemm_tiles,
        "16-column tiles per workgroup int4_gemm launches with",
        pybind11::arg("N"), pybind11::arg("M"));
  m.def("int4_moe_gemm", &int4_moe_gemm,
        "y[t*k+j] = x[(t*k+j) / row_div] @ W[selected[t,j]]^T over packed int4 "
        "experts, T <= 64; n_tiles = 0 takes int4_moe_plan's",
        pybind11::arg("y"), pybind11::arg("x"), pybind11::arg("selected"),
        pybind11::arg("table"), pybind11::arg("row_div"), pybind11::arg("E"),
        pybind11::arg("N"), pybind11::arg("K"), pybind11::arg("group"),
        pybind11::arg("n_tiles") = 0);
  m.def("moe_combine", &moe_combine,
        "out[t] = sum_j weights[t,j] * y[t*k+j] in ascending expert id, bf16 "
        "steps; ids outside [0, E) are skipped (E = 0: no upper limit)",
        pybind11::arg("out"), pybind11::arg("y"), pybind11::arg("selected"),
        pybind11::arg("weights"), pybind11::arg("E") = 0);
  m.def("int4_moe_plan", &int4_moe_plan,
        "(16-row tiles, 16-column tiles per workgroup) int4_moe_gemm launches "
        "with", pybind11::arg("N"), pybind11::arg("T"), pybind11::arg("E"),
        pybind11::arg("k"));
  m.def("fp8_moe_gemm", &fp8_moe_gemm,
        "y[t*k+j] = bf16(xq[(t*k+j) / row_div] @ wq_e^T * xs * ws_e), e = "
        "selected[t,j], over e4m3 experts, T <= 64; n_tiles = 0 takes "
        "fp8_moe_plan's",
        pybind11::arg("y"), pybind11::arg("xq"), pybind11::arg("xs"),
        pybind11::arg("selected"), pybind11::arg("table"),
        pybind11::arg("row_div"), pybind11::arg("E"), pybind11::arg("N"),
        pybind11::arg("K"), pybind11::arg("n_tiles") = 0);
  m.def("fp8_moe_plan", &fp8_moe_plan,
        "(16-row tiles, 16-column tiles per workgroup) fp8_moe_gemm launches "
        "with", pybind11::arg("N"), pybind11::arg("T"), pybind11::arg("E"),
        pybind11::arg("k"));
  m.def("greedy_sample", &greedy_sample, "argmax sampling");
  m.def("gumbel_sample", &gumbel_sample, "temperature sampling (hash RNG)");
  m.def("greedy_sample_logprob", &greedy_sample_logprob,
        "argmax sampling + the token's logprob and the row logsumexp");
  m.def("gumbel_sample_logprob", &gumbel_sample_logprob,
        "temperature sampling + the token's logprob and the row logsumexp");
  m.def("token_logprobs", &token_logprobs,
        "logprob of given tokens and the row logsumexp, one launch");
  m.def("rmsnorm_fp8", &rmsnorm_fp8, "rmsnorm with fused fp8 row quant");
  m.def("fused_add_rmsnorm_fp8", &fused_add_rmsnorm_fp8,
        "residual add + rmsnorm with fused fp8 row quant");
  m.def("fused_add_rmsnorm_fp8_div", &fused_add_rmsnorm_fp8_div,
        "residual add + rmsnorm, then the division-form fp8 row quant of its "
        "bf16 row (lm_head's input)");
  m.def("embed_rmsnorm_fp8", &embed_rmsnorm_fp8,
        "embedding gather + rmsnorm with fused fp8 row quant (layer 0)");
  m.def("silu_and_mul_fp8", &silu_and_mul_fp8, "SwiGLU with fused fp8 quant");
  m.def("quant_fp8", &quant_fp8, "bf16 -> fp8 row quant");
  m.def("quant_fp8_div", &quant_fp8_div,
        "bf16 -> fp8 row quant, division form (Fp8Linear.forward)");
  m.def("nucleus_stats", &nucleus_stats, "per-row softmax max + Z");
  m.def("nucleus_accept", &nucleus_accept,
        "nucleus membership of sampled tokens (mass above < p, rank < k)");
  m.def("xgmi_alloc", &xgmi_alloc, "allocate + export the IPC comm buffer");
  m.def("xgmi_connect", &xgmi_connect, "open peer IPC buffers");
  m.def("xgmi_fused_allreduce_add_rmsnorm", &xgmi_fused_allreduce_add_rmsnorm,
        "one-shot xGMI all-reduce fused with residual add + RMSNorm");
  m.def("xgmi_error_count", &xgmi_error_count, "spin-wait timeout count");
  m.def("xgmi_max_elems", &xgmi_max_elems, "one-shot capacity (bf16 elems)");
  m.def("xgmi_shutdown", &xgmi_shutdown, "free/close comm buffers");
  m.def("sgmv", &sgmv, "segmented gather LoRA apply (one adapter segment)");
  register_chwbl(m);
}
