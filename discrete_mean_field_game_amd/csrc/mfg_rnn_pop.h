// The RNN baseline as a population (mfg_rnn_fit_pop, include/mfg_hip.h): the third arm of the paper's comparison, which the
// reference keeps as text files only -- it writes the network's training file (process.py:4-22), reads its predictions back
// (read_rnn, mfg_ac2.py:757-761) and hard-codes its scores (plots.py:29-30).  K independent one-layer LSTMs with a softmax head,
// each with its own hidden size, learning rate, weight decay, clip, epochs and day lists, in two launches.
//   k_rnn_train     one workgroup per model, ALL its epochs in one launch (no launch per epoch, no grid-wide barrier).  Per epoch:
//                   the input half of every gate for all hours at once, the forward chain over the Hd - 1 hours (two barriers an
//                   hour: gates, then cell and hidden state), the head, softmax and loss of all hours at once, the head's
//                   gradient into the hidden states, the backward chain (one barrier an hour), every weight gradient as one sum
//                   over (hour, day), the norms, the update.  After every eval_every-th epoch and the last: the free-running
//                   forecast of the validation days (rnn_forecast) and the selection.
//   k_rnn_forecast  one workgroup per model: rnn_forecast of the test days from the selected weights, per-day values, mean and std.
// Per hour the model's days are a batch (columns, padded to a multiple of 4 with exact zeros), so the heavy pieces are small
// matrix products.  They run on the fp64 VECTOR unit, a thread per 1 x 4 tile of the product: the f64 matrix instruction of gfx950
// issues at the vector fp64 rate (profiles/r03_mfma_f64_rate.txt), so it buys no arithmetic here, while its 16-column tile would pad
// 13 days to 16 and its operand layouts would cost a transpose of the hidden state every hour; what bounds an epoch at each H is
// measured in DESIGN.md, "The RNN baseline": where the operands come from, not the multiply-adds.
// Weights and the gradient accumulator live in LDS when both fit (2 W(H, d) <= RNN_LDS_DOUBLES), else in the model's slice.
// A model's slice (doubles, every section rounded up to 4): m | v | best | w, g (used when not resident) | X [Hd][d][NP] the
// training days, hour-major, columns = days | A [T][4H][NP] gates, then their gradients | C, Hs, DH [T][H][NP] | Z [T][d][NP]
// logits, then their gradients | DC [H][NP] | losses [T n_train] | the forecast's x [d][NF], h, c [H][NF], gates [4H][NF], logits
// [d][NF], future [NF][Hd][d], row values [NF Hd][2], per-day values [NF][4].  T = Hd - 1, NP = n_train and NF = max(n_val,
// n_test, 1) rounded up to 4.  Every word that is read was written by this call: the contents are scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"

namespace mfg {

constexpr int RNN_MAX_D = 64, RNN_MAX_H = 64, RNN_MAX_HOURS = 64, RNN_MAX_DAYS = 64;
#ifndef MFG_RNN_THREADS
#define MFG_RNN_THREADS 1024   // (a side build may try another workgroup size: the summation orders documented in mfg_hip.h are those of 1024)
#endif
constexpr int RNN_THREADS = MFG_RNN_THREADS;
constexpr int RNN_LDS_DOUBLES = 18944;   // 148 KB of the CU's 160 KB for the resident weights and gradient

__host__ __device__ inline int rnn_up4(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int rnn_weights(int H, int d) { return 4 * H * (d + H + 1) + d * (H + 1); }
// the checks of a model: after every eval_every-th epoch and after the last
__host__ __device__ inline int rnn_checks(int epochs, int n_val, int eval_every) {
  return n_val > 0 ? (epochs + eval_every - 1) / eval_every : 0;
}

// offsets, in doubles, of the sections of a model's slice
struct RnnLayout {
  int64_t m, v, best, w, g, X, A, C, Hs, DH, Z, DC, losses, fx, fh, fc, fa, fz, fut, rows, pd, total;
  int NP, NF;
};
__host__ __device__ inline RnnLayout rnn_layout(int d, int H, int Hd, int n_train, int n_val, int n_test) {
  RnnLayout L;
  const int64_t W = rnn_up4(rnn_weights(H, d)), T = Hd - 1;
  int nf = n_val > n_test ? n_val : n_test;
  L.NP = rnn_up4(n_train);
  L.NF = rnn_up4(nf < 1 ? 1 : nf);
  int64_t at = 0;
  auto take = [&](int64_t n) { const int64_t o = at; at += (n + 3) & ~(int64_t)3; return o; };
  L.m = take(W), L.v = take(W), L.best = take(W), L.w = take(W), L.g = take(W);
  L.X = take((int64_t)Hd * d * L.NP);
  L.A = take(T * 4 * H * L.NP);
  L.C = take(T * H * L.NP), L.Hs = take(T * H * L.NP), L.DH = take(T * H * L.NP);
  L.Z = take(T * d * L.NP);
  L.DC = take((int64_t)H * L.NP);
  L.losses = take(T * L.NP);
  L.fx = take((int64_t)d * L.NF), L.fh = take((int64_t)H * L.NF), L.fc = take((int64_t)H * L.NF);
  L.fa = take((int64_t)4 * H * L.NF), L.fz = take((int64_t)d * L.NF);
  L.fut = take((int64_t)L.NF * Hd * d), L.rows = take((int64_t)L.NF * Hd * 2), L.pd = take((int64_t)L.NF * 4);
  L.total = at;
  return L;
}
inline size_t rnn_model_bytes(int d, int H, int Hd, int n_train, int n_val, int n_test) {
  return ((size_t)rnn_layout(d, H, Hd, n_train, n_val, n_test).total * 8 + 255) / 256 * 256;
}

void launch_rnn_fit(const mfg_rnn_fit_t& f, hipStream_t st);

}  // namespace mfg
