// The two kernels of mfg_rnn_fit_pop and its entry points (mfg_rnn_pop.h, include/mfg_hip.h).
#include <math.h>

#include "mfg_host.h"
#include "mfg_rnn_pop.h"
#include "mfg_var_pop.h"

namespace mfg {

constexpr int RNN_WAVES = RNN_THREADS / 64;

// the packed weights of a model: Wx [G, d] at 0, Wh [G, H] at oWh, b [G] at ob, Wo [d, H] at oWo, bo [d] at obo; G = 4H
struct RnnModel {
  int d, H, G, Hd, T, W;
  int oWh, ob, oWo, obo;
};

__device__ __forceinline__ RnnModel rnn_model(int d, int H, int Hd) {
  RnnModel M;
  M.d = d, M.H = H, M.G = 4 * H, M.Hd = Hd, M.T = Hd - 1, M.W = rnn_weights(H, d);
  M.oWh = M.G * d, M.ob = M.oWh + M.G * H, M.oWo = M.ob + M.G, M.obo = M.oWo + d * H;
  return M;
}

__device__ __forceinline__ double rnn_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

// row r of the gates: i, f, o logistic, g (the third block) tanh
__device__ __forceinline__ double rnn_gate(double a, int r, int H) { return (r >= 2 * H && r < 3 * H) ? tanh(a) : rnn_sigmoid(a); }

struct double4v {
  double v[4];
};
// four consecutive days of one row.  Rows start at multiples of 4 doubles of a workspace that is only 8-byte aligned: the pair
// type carries that alignment, so the compiler picks loads and stores that are legal for it.
struct alignas(8) rnn_pair {
  double x, y;
};
__device__ __forceinline__ double4v rnn_load4(const double* p) {
  const rnn_pair lo = *reinterpret_cast<const rnn_pair*>(p), hi = *reinterpret_cast<const rnn_pair*>(p + 2);
  return {{lo.x, lo.y, hi.x, hi.y}};
}
__device__ __forceinline__ void rnn_store4(double* p, const double (&a)[4]) {
  *reinterpret_cast<rnn_pair*>(p) = rnn_pair{a[0], a[1]};
  *reinterpret_cast<rnn_pair*>(p + 2) = rnn_pair{a[2], a[3]};
}

// acc[c] += sum_{i < n} w[i ws] b[i NP + c] for the four days c, i ascending
__device__ __forceinline__ void rnn_dot4(double (&acc)[4], const double* w, int ws, const double* b, int NP, int n) {
  for (int i = 0; i < n; ++i) {
    const double wv = w[i * ws];
    const double4v x = rnn_load4(b + i * NP);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = fma(wv, x.v[c], acc[c]);
  }
}

// The sum of x over the workgroup, the same bits in every thread: an xor butterfly within each wave, the 16 wave sums in wave
// order.  Ends behind a barrier.
__device__ __forceinline__ double rnn_block_sum(double x, double* red) {
  x = var_wave_sum(x);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int q = 1; q < RNN_WAVES; ++q) s += red[q];
  __syncthreads();
  return s;
}

__device__ __forceinline__ const double* rnn_day_row(const mfg_rnn_fit_t& f, const int32_t* list, int n, int hour) {
  return f.days + ((int64_t)var_day(list[n], f.D) * f.Hd + hour) * f.d;
}

struct RnnScratch {
  double *fx, *fh, *fc, *fa, *fz, *rows, *pd;
};

// The free-running forecast of the Nd days of `list` from the weights w, and its per-day values: every day starts from its
// observed hour 0 with zero state, the model's own output is fed back for Hd - 1 hours.  future [Nd][Hd][d], hour 0 the observed
// row; s.pd [Nd][4] = l1_final, l1_mean, JSD_final, JSD_mean.  The days are the columns of every buffer (NP = Nd rounded up to 4,
// padded columns zero).  Called by every thread of the workgroup; ends behind a barrier.
__device__ void rnn_forecast(const mfg_rnn_fit_t& f, const RnnModel& M, const double* w, const int32_t* list, int Nd, double* future,
                             const RnnScratch& s) {
  const int tid = threadIdx.x, d = M.d, H = M.H, G = M.G, Hd = M.Hd;
  const int NP = rnn_up4(Nd), NT = NP >> 2;
  for (int e = tid; e < d * NP; e += RNN_THREADS) {
    const int j = e / NP, n = e - j * NP;
    const double y = n < Nd ? rnn_day_row(f, list, n, 0)[j] : 0.0;
    s.fx[e] = y;
    if (n < Nd) future[(int64_t)n * Hd * d + j] = y;
  }
  __syncthreads();
  for (int t = 0; t < Hd - 1; ++t) {
    for (int e = tid; e < G * NT; e += RNN_THREADS) {
      const int r = e / NT, n0 = (e - r * NT) * 4;
      const double b = w[M.ob + r];
      double acc[4] = {b, b, b, b};
      rnn_dot4(acc, w + r * d, 1, s.fx + n0, NP, d);
      if (t > 0) rnn_dot4(acc, w + M.oWh + r * H, 1, s.fh + n0, NP, H);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = rnn_gate(acc[c], r, H);
      rnn_store4(s.fa + r * NP + n0, acc);
    }
    __syncthreads();
    for (int e = tid; e < H * NP; e += RNN_THREADS) {
      const double gi = s.fa[e], gf = s.fa[H * NP + e], gg = s.fa[2 * H * NP + e], go = s.fa[3 * H * NP + e];
      const double c = fma(gf, t > 0 ? s.fc[e] : 0.0, gi * gg);
      s.fc[e] = c;
      s.fh[e] = go * tanh(c);
    }
    __syncthreads();
    for (int e = tid; e < d * NT; e += RNN_THREADS) {
      const int j = e / NT, n0 = (e - j * NT) * 4;
      const double b = w[M.obo + j];
      double acc[4] = {b, b, b, b};
      rnn_dot4(acc, w + M.oWo + j * H, 1, s.fh + n0, NP, H);
      rnn_store4(s.fz + j * NP + n0, acc);
    }
    __syncthreads();
    for (int n = tid; n < NP; n += RNN_THREADS) {
      if (n < Nd) {
        double mx = s.fz[n];
        for (int j = 1; j < d; ++j) mx = fmax(mx, s.fz[j * NP + n]);
        double se = 0.0;
        for (int j = 0; j < d; ++j) se += exp(s.fz[j * NP + n] - mx);
        for (int j = 0; j < d; ++j) {
          const double y = exp(s.fz[j * NP + n] - mx) / se;
          s.fx[j * NP + n] = y;
          future[((int64_t)n * Hd + t + 1) * d + j] = y;
        }
      } else {
        for (int j = 0; j < d; ++j) s.fx[j * NP + n] = 0.0;
      }
    }
    __syncthreads();
  }
  // L1 and JSD of every (day, hour) row, a row per wave; then a thread per day, hours in order
  for (int row = tid >> 6; row < Nd * Hd; row += RNN_WAVES) {
    const int n = row / Hd, hour = row - n * Hd;
    double l1, jsd;
    var_row_metrics(rnn_day_row(f, list, n, hour), future + (int64_t)row * d, d, l1, jsd);
    if ((tid & 63) == 0) s.rows[2 * row] = l1, s.rows[2 * row + 1] = jsd;
  }
  __syncthreads();
  if (tid < Nd) {
    double l1 = 0.0, jsd = 0.0;
    for (int h = 0; h < Hd; ++h) l1 += s.rows[2 * (tid * Hd + h)], jsd += s.rows[2 * (tid * Hd + h) + 1];
    s.pd[4 * tid] = s.rows[2 * (tid * Hd + Hd - 1)];
    s.pd[4 * tid + 1] = l1 / (double)Hd;
    s.pd[4 * tid + 2] = s.rows[2 * (tid * Hd + Hd - 1) + 1];
    s.pd[4 * tid + 3] = jsd / (double)Hd;
  }
  __syncthreads();
}

__device__ __forceinline__ RnnScratch rnn_scratch(double* ws, const RnnLayout& L) {
  return {ws + L.fx, ws + L.fh, ws + L.fc, ws + L.fa, ws + L.fz, ws + L.rows, ws + L.pd};
}

// ---- one workgroup, model blockIdx.x: every epoch of the model
__global__ __launch_bounds__(RNN_THREADS) void k_rnn_train(mfg_rnn_fit_t f) {
  const int k = blockIdx.x, tid = threadIdx.x;
  const mfg_rnn_model_t mo = f.models[k];
  const int d = f.d, H = mo.hidden, Hd = f.Hd, N = mo.n_train;
  const RnnModel M = rnn_model(d, H, Hd);
  const RnnLayout L = rnn_layout(d, H, Hd, N, mo.n_val, mo.n_test);
  const int G = M.G, T = M.T, W = M.W, NP = L.NP, NT = NP >> 2;
  double* ws = reinterpret_cast<double*>(reinterpret_cast<char*>(f.workspace) + mo.ws_offset);
  const int32_t* tr = f.train_idx + (int64_t)k * f.train_stride;
  const int32_t* va = f.val_idx + (int64_t)k * f.val_stride;
  const int32_t* te = f.test_idx + (int64_t)k * f.test_stride;
  double* w_out = f.weights + (int64_t)k * f.W_max;
  double* loss_out = f.loss + (int64_t)k * f.E_max;
  double* val_out = f.val ? f.val + (int64_t)k * f.C_max : nullptr;

  __shared__ double arena[RNN_LDS_DOUBLES];
  __shared__ double red[RNN_WAVES];
  __shared__ int bad;
  // weights and gradient accumulator: on chip when both fit, else in the slice
  const bool resident = 2 * rnn_up4(W) <= RNN_LDS_DOUBLES;
  double* w = resident ? arena : ws + L.w;
  double* g = resident ? arena + rnn_up4(W) : ws + L.g;
  double *am = ws + L.m, *av = ws + L.v, *best = ws + L.best;
  double *X = ws + L.X, *A = ws + L.A, *C = ws + L.C, *Hs = ws + L.Hs, *DH = ws + L.DH, *Z = ws + L.Z, *DC = ws + L.DC;
  double* losses = ws + L.losses;
  const RnnScratch scratch = rnn_scratch(ws, L);

  if (tid == 0) bad = 0;
  __syncthreads();
  // what the model reads: its day indices, every value of its days, its initial weights
  int mine = 0;
  for (int q = 0; q < 3; ++q) {
    const int32_t* list = q == 0 ? tr : (q == 1 ? va : te);
    const int cnt = q == 0 ? N : (q == 1 ? mo.n_val : mo.n_test);
    for (int i = tid; i < cnt; i += RNN_THREADS) mine |= list[i] < 0 || list[i] >= f.D;
    for (int e = tid; e < cnt * Hd * d; e += RNN_THREADS) {
      const int n = e / (Hd * d);
      mine |= !isfinite(rnn_day_row(f, list, n, 0)[e - n * Hd * d]);
    }
  }
  const double* w0 = f.w0 + (int64_t)k * f.W_max;
  for (int i = tid; i < W; i += RNN_THREADS) mine |= !isfinite(w0[i]);
  if (mine) atomicOr(&bad, 1);
  __syncthreads();
  int status = bad ? MFG_RNN_NONFINITE : 0;

  int best_epoch = 0;
  if (!status) {
    for (int i = tid; i < W; i += RNN_THREADS) w[i] = w0[i], am[i] = 0.0, av[i] = 0.0;
    // the training days, hour-major, a day per column; padded columns exact zeros
    for (int e = tid; e < Hd * d * NP; e += RNN_THREADS) {
      const int n = e % NP, tj = e / NP, t = tj / d, j = tj - t * d;
      X[e] = n < N ? rnn_day_row(f, tr, n, t)[j] : 0.0;
    }
    for (int e = mo.epochs + tid; e < f.E_max; e += RNN_THREADS) loss_out[e] = NAN;
    for (int e = tid; e < f.C_max; e += RNN_THREADS) val_out[e] = NAN;
    __syncthreads();

    const double count = (double)(N * T);
    double b1t = 1.0, b2t = 1.0, best_val = INFINITY;
    int check = 0;
    for (int ep = 1; ep <= mo.epochs; ++ep) {
      // the input half of every gate, all hours at once: A[t][r][n] = b[r] + sum_j Wx[r][j] x[n, t, j]
      for (int e = tid; e < T * G * NT; e += RNN_THREADS) {
        const int t = e / (G * NT), rem = e - t * G * NT, r = rem / NT, n0 = (rem - r * NT) * 4;
        const double b = w[M.ob + r];
        double acc[4] = {b, b, b, b};
        rnn_dot4(acc, w + r * d, 1, X + t * d * NP + n0, NP, d);
        rnn_store4(A + (t * G + r) * NP + n0, acc);
      }
      double sq = 0.0;
      for (int i = tid; i < W; i += RNN_THREADS) sq = fma(w[i], w[i], sq);
      const double wnorm2 = rnn_block_sum(sq, red);
      // the forward chain: the hidden half of the gates, then cell and hidden state
      for (int t = 0; t < T; ++t) {
        for (int e = tid; e < G * NT; e += RNN_THREADS) {
          const int r = e / NT, n0 = (e - r * NT) * 4;
          double* a = A + (t * G + r) * NP + n0;
          const double4v a0 = rnn_load4(a);
          double acc[4] = {a0.v[0], a0.v[1], a0.v[2], a0.v[3]};
          if (t > 0) rnn_dot4(acc, w + M.oWh + r * H, 1, Hs + (t - 1) * H * NP + n0, NP, H);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] = rnn_gate(acc[c], r, H);
          rnn_store4(a, acc);
        }
        __syncthreads();
        for (int e = tid; e < H * NP; e += RNN_THREADS) {
          const double* a = A + t * G * NP + e;
          const double gi = a[0], gf = a[H * NP], gg = a[2 * H * NP], go = a[3 * H * NP];
          const double c = fma(gf, t > 0 ? C[(t - 1) * H * NP + e] : 0.0, gi * gg);
          C[t * H * NP + e] = c;
          Hs[t * H * NP + e] = go * tanh(c);
        }
        __syncthreads();
      }
      // the head, all hours at once: Z[t][j][n] = bo[j] + sum_k Wo[j][k] h[t][k][n]
      for (int e = tid; e < T * d * NT; e += RNN_THREADS) {
        const int t = e / (d * NT), rem = e - t * d * NT, j = rem / NT, n0 = (rem - j * NT) * 4;
        const double b = w[M.obo + j];
        double acc[4] = {b, b, b, b};
        rnn_dot4(acc, w + M.oWo + j * H, 1, Hs + t * H * NP + n0, NP, H);
        rnn_store4(Z + (t * d + j) * NP + n0, acc);
      }
      __syncthreads();
      // softmax, the loss of every (hour, day), and dL/dz in place of z (padded days: zeros)
      for (int e = tid; e < T * NP; e += RNN_THREADS) {
        const int t = e / NP, n = e - t * NP;
        double* z = Z + t * d * NP + n;
        if (n < N) {
          const double* y = X + (t + 1) * d * NP + n;
          double mx = z[0];
          for (int j = 1; j < d; ++j) mx = fmax(mx, z[j * NP]);
          double se = 0.0, sy = 0.0;
          for (int j = 0; j < d; ++j) se += exp(z[j * NP] - mx), sy += y[j * NP];
          const double lse = mx + log(se);
          double l = 0.0;
          for (int j = 0; j < d; ++j) {
            const double lp = z[j * NP] - lse;
            l = fma(-y[j * NP], lp, l);
            z[j * NP] = (exp(lp) * sy - y[j * NP]) / count;
          }
          losses[t * N + n] = l;
        } else {
          for (int j = 0; j < d; ++j) z[j * NP] = 0.0;
        }
      }
      __syncthreads();
      // the head's gradient into the hidden states, all hours at once: DH[t][k][n] = sum_j Wo[j][k] dz[t][j][n]
      for (int e = tid; e < T * H * NT; e += RNN_THREADS) {
        const int t = e / (H * NT), rem = e - t * H * NT, kk = rem / NT, n0 = (rem - kk * NT) * 4;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        rnn_dot4(acc, w + M.oWo + kk, H, Z + t * d * NP + n0, NP, d);
        rnn_store4(DH + (t * H + kk) * NP + n0, acc);
      }
      double ls = 0.0;
      for (int i = tid; i < T * N; i += RNN_THREADS) ls += losses[i];
      const double loss = rnn_block_sum(ls, red) / count + 0.5 * mo.wd * wnorm2;
      // the backward chain.  Four lanes share a 1 x 4 tile of dh = Wh' dA[t + 1], one gate block each; the partial sums are added
      // in gate order, then lane q takes day q of the tile through the cell: dA[t] replaces the gates of hour t.
      for (int t = T - 1; t >= 0; --t) {
        for (int base = 0; base < H * NT * 4; base += RNN_THREADS) {
          const int e = base + tid, q = e & 3, tile = e >> 2;
          const bool on = tile < H * NT;
          const int kk = on ? tile / NT : 0, n0 = on ? (tile - kk * NT) * 4 : 0;
          double acc[4] = {0.0, 0.0, 0.0, 0.0};
          if (on && t < T - 1) rnn_dot4(acc, w + M.oWh + q * H * H + kk, H, A + ((t + 1) * G + q * H) * NP + n0, NP, H);
          const int lane0 = (tid & 63) & ~3;
          double s = 0.0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const double p0 = __shfl(acc[c], lane0), p1 = __shfl(acc[c], lane0 + 1), p2 = __shfl(acc[c], lane0 + 2),
                         p3 = __shfl(acc[c], lane0 + 3);
            const double sc = ((p0 + p1) + p2) + p3;
            s = c == q ? sc : s;
          }
          if (on) {
            const int at = kk * NP + n0 + q;
            double* a = A + t * G * NP + at;
            const double gi = a[0], gf = a[H * NP], gg = a[2 * H * NP], go = a[3 * H * NP];
            const double dh = DH[t * H * NP + at] + s;
            const double tc = tanh(C[t * H * NP + at]);
            const double cp = t > 0 ? C[(t - 1) * H * NP + at] : 0.0;
            const double dc = fma(dh * go, 1.0 - tc * tc, t < T - 1 ? DC[at] : 0.0);
            a[0] = dc * gg * (gi * (1.0 - gi));
            a[H * NP] = dc * cp * (gf * (1.0 - gf));
            a[2 * H * NP] = dc * gi * (1.0 - gg * gg);
            a[3 * H * NP] = dh * tc * (go * (1.0 - go));
            DC[at] = dc * gf;
          }
        }
        __syncthreads();
      }
      // every weight gradient as one sum over (hour, day), hours ascending.  Gate rows, four rows a thread: column c < d is Wx
      // (against x[t]), c < d + H is Wh (against h[t - 1], from hour 1), c = d + H the bias (against ones).
      const int cols = d + H + 1;
      for (int e = tid; e < (G >> 2) * cols; e += RNN_THREADS) {
        const int r0 = (e / cols) * 4, c = e % cols;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int t = (c >= d && c < d + H) ? 1 : 0; t < T; ++t) {
          const double* bp = c < d ? X + (t * d + c) * NP : (c < d + H ? Hs + ((t - 1) * H + c - d) * NP : nullptr);
          for (int n0 = 0; n0 < NP; n0 += 4) {
            const double4v b = bp ? rnn_load4(bp + n0) : double4v{{1.0, 1.0, 1.0, 1.0}};
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              const double4v a = rnn_load4(A + (t * G + r0 + rr) * NP + n0);
#pragma unroll
              for (int i = 0; i < 4; ++i) acc[rr] = fma(a.v[i], b.v[i], acc[rr]);
            }
          }
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int r = r0 + rr;
          const int idx = c < d ? r * d + c : (c < d + H ? M.oWh + r * H + c - d : M.ob + r);
          g[idx] = fma(mo.wd, w[idx], acc[rr]);
        }
      }
      // head rows: Wo[j][c] against h[t], c = H the bias
      for (int e = tid; e < d * (H + 1); e += RNN_THREADS) {
        const int j = e / (H + 1), c = e - j * (H + 1);
        double acc = 0.0;
        for (int t = 0; t < T; ++t) {
          const double* zp = Z + (t * d + j) * NP;
          const double* bp = c < H ? Hs + (t * H + c) * NP : nullptr;
          for (int n0 = 0; n0 < NP; n0 += 4) {
            const double4v a = rnn_load4(zp + n0);
            const double4v b = bp ? rnn_load4(bp + n0) : double4v{{1.0, 1.0, 1.0, 1.0}};
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = fma(a.v[i], b.v[i], acc);
          }
        }
        const int idx = c < H ? M.oWo + j * H + c : M.obo + j;
        g[idx] = fma(mo.wd, w[idx], acc);
      }
      __syncthreads();
      double gs = 0.0;
      for (int i = tid; i < W; i += RNN_THREADS) gs = fma(g[i], g[i], gs);
      const double gn = sqrt(rnn_block_sum(gs, red));
      if (!isfinite(loss) || !isfinite(gn)) {
        status = MFG_RNN_DIVERGED;
        break;
      }
      if (tid == 0) loss_out[ep - 1] = loss;
      const double scale = (mo.clip > 0.0 && gn > mo.clip) ? mo.clip / gn : 1.0;
      b1t *= 0.9, b2t *= 0.999;
      if (f.optimizer == MFG_RNN_ADAM) {
        const double step = mo.lr / (1.0 - b1t), root = sqrt(1.0 - b2t);
        for (int i = tid; i < W; i += RNN_THREADS) {
          const double gi = g[i] * scale;
          const double m = 0.9 * am[i] + (1.0 - 0.9) * gi;
          const double v = 0.999 * av[i] + (1.0 - 0.999) * (gi * gi);
          am[i] = m, av[i] = v;
          w[i] -= step * (m / (sqrt(v) / root + 1e-8));
        }
      } else {
        for (int i = tid; i < W; i += RNN_THREADS) w[i] -= mo.lr * (g[i] * scale);
      }
      __syncthreads();
      // held-out selection
      if (mo.n_val > 0 && (ep % f.eval_every == 0 || ep == mo.epochs)) {
        rnn_forecast(f, M, w, va, mo.n_val, ws + L.fut, scratch);
        double vm = 0.0;
        for (int n = 0; n < mo.n_val; ++n) vm += scratch.pd[4 * n + 3];
        vm /= (double)mo.n_val;
        if (!isfinite(vm)) {
          status = MFG_RNN_DIVERGED;
          break;
        }
        if (tid == 0) val_out[check] = vm;
        ++check;
        if (vm < best_val) {
          best_val = vm, best_epoch = ep;
          for (int i = tid; i < W; i += RNN_THREADS) best[i] = w[i];
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();
  if (status) {
    for (int e = tid; e < f.W_max; e += RNN_THREADS) w_out[e] = NAN;
    for (int e = tid; e < f.E_max; e += RNN_THREADS) loss_out[e] = NAN;
    for (int e = tid; e < f.C_max; e += RNN_THREADS) val_out[e] = NAN;
    if (tid == 0) f.best_epoch[k] = 0, f.status[k] = status;
    return;
  }
  const double* chosen = mo.n_val > 0 ? best : w;
  for (int e = tid; e < f.W_max; e += RNN_THREADS) w_out[e] = e < W ? chosen[e] : 0.0;
  if (tid == 0) f.best_epoch[k] = mo.n_val > 0 ? best_epoch : mo.epochs, f.status[k] = 0;
}

// ---- one workgroup, model blockIdx.x: the test forecast from the selected weights, per-day values, mean and std
__global__ __launch_bounds__(RNN_THREADS) void k_rnn_forecast(mfg_rnn_fit_t f) {
  const int k = blockIdx.x, tid = threadIdx.x;
  const mfg_rnn_model_t mo = f.models[k];
  const int d = f.d, Hd = f.Hd, Nt = mo.n_test;
  if (f.test_stride == 0) {
    if (tid < 8) f.metrics[(int64_t)k * 8 + tid] = NAN;
    return;
  }
  double* future = f.future + (int64_t)k * f.test_stride * Hd * d;
  double* per_day = f.per_day + (int64_t)k * f.test_stride * 4;
  if (f.status[k] != 0) {
    for (int e = tid; e < f.test_stride * Hd * d; e += RNN_THREADS) future[e] = NAN;
    for (int e = tid; e < f.test_stride * 4; e += RNN_THREADS) per_day[e] = NAN;
    if (tid < 8) f.metrics[(int64_t)k * 8 + tid] = NAN;
    return;
  }
  const RnnModel M = rnn_model(d, mo.hidden, Hd);
  const RnnLayout L = rnn_layout(d, mo.hidden, Hd, mo.n_train, mo.n_val, mo.n_test);
  double* ws = reinterpret_cast<double*>(reinterpret_cast<char*>(f.workspace) + mo.ws_offset);
  const RnnScratch scratch = rnn_scratch(ws, L);
  if (Nt > 0) rnn_forecast(f, M, f.weights + (int64_t)k * f.W_max, f.test_idx + (int64_t)k * f.test_stride, Nt, future, scratch);
  for (int e = tid; e < f.test_stride * 4; e += RNN_THREADS) per_day[e] = e < Nt * 4 ? scratch.pd[e] : 0.0;
  for (int e = Nt * Hd * d + tid; e < f.test_stride * Hd * d; e += RNN_THREADS) future[e] = 0.0;
  if (tid < 4) {
    // mean and np.std (ddof 0) over the test days, in day order
    double mean = NAN, sd = NAN;
    if (Nt > 0) {
      double a = 0.0;
      for (int j = 0; j < Nt; ++j) a += scratch.pd[4 * j + tid];
      mean = a / (double)Nt;
      double q = 0.0;
      for (int j = 0; j < Nt; ++j) q = fma(scratch.pd[4 * j + tid] - mean, scratch.pd[4 * j + tid] - mean, q);
      sd = sqrt(q / (double)Nt);
    }
    f.metrics[(int64_t)k * 8 + 2 * tid] = mean;
    f.metrics[(int64_t)k * 8 + 2 * tid + 1] = sd;
  }
}

void launch_rnn_fit(const mfg_rnn_fit_t& f, hipStream_t st) {
  hipLaunchKernelGGL(k_rnn_train, dim3((unsigned)f.K), dim3(RNN_THREADS), 0, st, f);
  hipLaunchKernelGGL(k_rnn_forecast, dim3((unsigned)f.K), dim3(RNN_THREADS), 0, st, f);
}

// NULL when the record is inside the limits of include/mfg_hip.h, else what is wrong with it
static const char* rnn_model_error(const mfg_rnn_model_t& mo) {
  if (mo.hidden < 4 || mo.hidden > RNN_MAX_H || (mo.hidden & 3)) return "hidden size not a multiple of 4 in [4, 64]";
  if (mo.epochs < 1 || mo.epochs > MFG_RNN_MAX_EPOCHS) return "epochs outside [1, 65535]";
  if (mo.n_train < 1 || mo.n_train > RNN_MAX_DAYS) return "training days outside [1, 64]";
  if (mo.n_val < 0 || mo.n_val > RNN_MAX_DAYS) return "validation days outside [0, 64]";
  if (mo.n_test < 0 || mo.n_test > RNN_MAX_DAYS) return "test days outside [0, 64]";
  if (!(mo.lr > 0.0) || !std::isfinite(mo.lr)) return "lr not finite and > 0";
  if (!(mo.wd >= 0.0) || !std::isfinite(mo.wd)) return "wd not finite and >= 0";
  if (!(mo.clip >= 0.0) || !std::isfinite(mo.clip)) return "clip not finite and >= 0";
  return nullptr;
}

}  // namespace mfg

using namespace mfg;

extern "C" size_t mfg_rnn_fit_workspace_bytes(int K, mfg_rnn_model_t* models_host, int d, int Hd) {
  if (K < 1 || !models_host || d < 2 || d > RNN_MAX_D || Hd < 2 || Hd > RNN_MAX_HOURS) return 0;
  size_t at = 0;
  for (int k = 0; k < K; ++k) {
    mfg_rnn_model_t& mo = models_host[k];
    if (rnn_model_error(mo)) return 0;
    mo.ws_offset = (int64_t)at;
    at += rnn_model_bytes(d, mo.hidden, Hd, mo.n_train, mo.n_val, mo.n_test);
  }
  return at;
}

extern "C" int mfg_rnn_fit_pop(const mfg_rnn_fit_t* fit) {
  REQUIRE(fit, "null descriptor");
  const mfg_rnn_fit_t& f = *fit;
  REQUIRE(f.K >= 1 && f.K <= MFG_POP_MAX_K, "population size K outside [1, MFG_POP_MAX_K]");
  REQUIRE(f.D >= 1, "D < 1");
  REQUIRE(f.Hd >= 2 && f.Hd <= RNN_MAX_HOURS, "Hd outside [2, 64]");
  REQUIRE(f.d >= 2 && f.d <= RNN_MAX_D, "d outside [2, 64]");
  REQUIRE(f.optimizer == MFG_RNN_ADAM || f.optimizer == MFG_RNN_SGD, "optimizer not MFG_RNN_ADAM or MFG_RNN_SGD");
  REQUIRE(f.eval_every >= 1, "eval_every < 1");
  REQUIRE(f.train_stride >= 1 && f.val_stride >= 0 && f.test_stride >= 0, "index table strides");
  REQUIRE(f.W_max >= 1 && f.E_max >= 1 && f.C_max >= 0, "W_max, E_max < 1 or C_max < 0");
  REQUIRE(f.days && f.models_host && f.models && f.train_idx && f.w0 && f.weights && f.loss && f.best_epoch && f.metrics &&
              f.status && f.workspace && (f.val_idx || f.val_stride == 0) && (f.test_idx || f.test_stride == 0) &&
              ((f.future && f.per_day) || f.test_stride == 0) && (f.val || f.C_max == 0),
          "null pointer");
  REQUIRE((reinterpret_cast<uintptr_t>(f.workspace) & 7) == 0, "workspace not 8-byte aligned");
  size_t at = 0;
  for (int k = 0; k < f.K; ++k) {
    const mfg_rnn_model_t& mo = f.models_host[k];
    if (const char* what = rnn_model_error(mo)) return fail(MFG_EINVAL, "rnn fit: model %d: %s", k, what);
    if (mo.n_train > f.train_stride || mo.n_val > f.val_stride || mo.n_test > f.test_stride)
      return fail(MFG_EINVAL, "rnn fit: model %d: more days than the index tables' strides", k);
    if (rnn_weights(mo.hidden, f.d) > f.W_max)
      return fail(MFG_EINVAL, "rnn fit: model %d: %d weights, W_max = %d", k, rnn_weights(mo.hidden, f.d), f.W_max);
    if (mo.epochs > f.E_max) return fail(MFG_EINVAL, "rnn fit: model %d: %d epochs, E_max = %d", k, mo.epochs, f.E_max);
    if (rnn_checks(mo.epochs, mo.n_val, f.eval_every) > f.C_max)
      return fail(MFG_EINVAL, "rnn fit: model %d: %d checks, C_max = %d", k, rnn_checks(mo.epochs, mo.n_val, f.eval_every), f.C_max);
    if (mo.ws_offset != (int64_t)at)
      return fail(MFG_EINVAL, "rnn fit: model %d: ws_offset is not the layout of mfg_rnn_fit_workspace_bytes", k);
    at += rnn_model_bytes(f.d, mo.hidden, f.Hd, mo.n_train, mo.n_val, mo.n_test);
  }
  if (f.workspace_bytes < at)
    return fail(MFG_EWORKSPACE, "rnn fit workspace: need %lld bytes, have %lld", (long long)at, (long long)f.workspace_bytes);
  launch_rnn_fit(f, S(f.stream));
  return check_launch("rnn_fit_pop");
}
