// hvk_api.h - C ABI of the veles_amd HIP kernel library (libhvk.so), used
// by the Python ops layer (ctypes) and by the native runtime (csrc/runtime).
#pragma once
#include <hip/hip_runtime.h>

extern "C" {
int hvk_gemm(int transA, int transB, int M, int N, int K, const void* A,
             int lda, const void* B, int ldb, void* C, int ldc, int out_f32,
             int atomic, float alpha, float beta, const float* bias,
             int bias_mode, int act, const void* aux, int ld_aux, int aux_act,
             int splits, float* bias_grad, hipStream_t s);
int hvk_gemm_splitk(int transA, int transB, int M, int N, int K,
                    const void* A, int lda, const void* B, int ldb, void* C,
                    int ldc, int out_f32, float alpha, const float* bias,
                    int act, const void* aux, int ld_aux, int aux_act,
                    int splits, float* ws, int ws_zero, hipStream_t s);
int hvk_conv_fwd(const void* X, const void* W, const float* bias, void* Y,
                 int N, int H, int Wd, int C, int OC, int KH, int KW, int sy,
                 int sx, int pt, int pl, int OH, int OW, int groups, int act,
                 hipStream_t s);
int hvk_conv_fwd_run(const void* X, const void* Wp, const float* bias, void* Y,
                     int N, int H, int Wd, int C, int OC, int KH, int KW,
                     int sy, int sx, int pt, int pl, int OH, int OW, int act,
                     hipStream_t s);
int hvk_pool_fwd(const void* x, void* y, int* argmax, int N, int H, int W,
                 int C, int OH, int OW, int ky, int kx, int sy, int sx, int pt,
                 int pl, int mode, hipStream_t s);
int hvk_lrn_fwd(const void* x, void* y, long long P, int C, int n, float alpha,
                float beta, float k, hipStream_t s);
// batch normalisation (batchnorm.hip): table [2][C] = scale, shift
int hvk_bn_partials(long long P, int C, int vec);
int hvk_bn_vec(const void* x, long long ldx, int C);
int hvk_bn_stats(const void* x, long long ldx, long long P, int C, int vec,
                 const float* gamma, const float* beta, float* running_mean,
                 float* running_var, float eps, float momentum, float* mean,
                 float* invstd, float* table, float* ws, hipStream_t s);
int hvk_bn_fold(const float* gamma, const float* beta,
                const float* running_mean, const float* running_var, int C,
                float eps, float* table, hipStream_t s);
int hvk_bn_apply(const void* x, long long ldx, void* y, long long ldy,
                 long long P, int C, const float* table, int act,
                 hipStream_t s);
int hvk_bn_bwd(const void* x, long long ldx, const void* err, long long lde,
               const void* y, long long ldy, const void* aux, long long lda,
               void* dx, long long lddx, long long P, int C, int vec,
               const float* gamma, const float* mean, const float* invstd,
               float* dgamma, float* dbeta, int accumulate, int act,
               int aux_act, float* coef, float* ws, hipStream_t s);
// layer normalisation and the residual add (layernorm.hip): bf16 [P][C] with
// row pitches in elements, r null: no residual; ws: 2 * C * hvk_ln_partials
int hvk_ln_partials(long long P, int C, int vec);
int hvk_ln_vec(const void* x, long long ldx, int C);
int hvk_ln_colsum(int mode);
int hvk_ln_fwd(const void* x, long long ldx, const void* r, long long ldr,
               void* y, long long ldy, long long P, int C, const float* gamma,
               const float* beta, float eps, float* mean, float* invstd,
               hipStream_t s);
int hvk_ln_bwd(const void* err, long long lde, const void* x, long long ldx,
               const void* r, long long ldr, void* dx, long long lddx,
               long long P, int C, int vec, const float* gamma,
               const float* mean, const float* invstd, float* dgamma,
               float* dbeta, int accumulate, int need_dx, float* ws,
               hipStream_t s);
int hvk_add(const void* a, long long lda, const void* b, long long ldb,
            void* out, long long ldo, long long P, int C, hipStream_t s);
// feed-forward activation passes (ffn.hip): bf16 [P][F] with row pitches in
// elements; act 0 gelu, 1 gelu_tanh, 2 strict relu; dut null: no du^T; ws:
// F * hvk_ffn_act_partials(P, F, dut != null) floats
int hvk_ffn_act_partials(long long P, int F, int transposed);
int hvk_ffn_act_fwd(const void* u, long long ldu, void* h, long long ldh,
                    long long P, int F, int act, hipStream_t s);
int hvk_ffn_act_bwd(const void* dh, long long lddh, const void* u,
                    long long ldu, void* du, long long lddu, void* dut,
                    long long lddut, long long P, int F, int act, float* db1,
                    int accumulate, float* ws, hipStream_t s);
// self-attention (attention.hip): bf16 [B][T][NH*D] views with row pitches,
// float32 lse / delta [B][NH][T]; D = 32, 64 or 128
int hvk_attn_tile(int which);
int hvk_attn_fwd(const void* q, long long ldq, const void* k, long long ldk,
                 const void* v, long long ldv, void* o, long long ldo,
                 float* lse, int B, int T, int NH, int D, int causal,
                 hipStream_t s);
int hvk_attn_bwd_delta(const void* dout, long long lddo, const void* o,
                       long long ldo, float* delta, int B, int T, int NH,
                       int D, hipStream_t s);
int hvk_attn_bwd_dkv(const void* q, long long ldq, const void* k,
                     long long ldk, const void* v, long long ldv,
                     const void* dout, long long lddo, const float* lse,
                     const float* delta, void* dk, long long lddk, void* dv,
                     long long lddv, int B, int T, int NH, int D, int causal,
                     hipStream_t s);
int hvk_attn_bwd_dq(const void* q, long long ldq, const void* k,
                    long long ldk, const void* v, long long ldv,
                    const void* dout, long long lddo, const float* lse,
                    const float* delta, void* dq, long long lddq, int B, int T,
                    int NH, int D, int causal, hipStream_t s);
int hvk_act_fwd(const void* x, int xdt, void* y, int ydt, long long n, int act,
                hipStream_t s);
int hvk_softmax_ce(const void* logits, int in_dt, int B, int C,
                   const int* labels, float scale, void* err, int err_dt,
                   float* probs, int* max_idx, float* metrics, int* confusion,
                   hipStream_t s);
int hvk_cast(const void* in, int idt, void* out, int odt, long long n,
             float scale, hipStream_t s);
}

enum { HVK_F32 = 0, HVK_BF16 = 1, HVK_U8 = 2, HVK_I32 = 3 };
