// Input gradients of the reward network: kernels, launch rules and the block's entry points (mfg_reward_grad.h,
// include/mfg_hip.h).
#include "mfg_reward_grad.h"

#include "mfg_core.h"
#include "mfg_host.h"
#include "mfg_irl_population.h"
#include "mfg_rn_common.h"

namespace mfg {

struct RnGradArgs {
  const float *state, *action;
  int64_t s_state, s_action, N;
  const float *c1w, *c1b, *c2w, *c2b, *w3, *b3, *w4, *b4, *wo, *bo;  // the launch's network (learner 0's / the shared one)
  int n3, n4;
  float keep_prob;
  int per_learner_net;
  int64_t s_net;
  const mfg_rn_geom_t* geom;
  const uint64_t* key;
  const int32_t* learner;
  uint64_t sample_offset;
  float *gs, *ga;  // per-sample destinations [K,N,d], [K,N,d,d]
};

// small weights in LDS, at fixed offsets (the largest geometry: n3 = 16, n4 = 32, d = 21)
constexpr int RG_O_C1W = 0, RG_O_C1B = 25, RG_O_C2W = 26, RG_O_C2B = 44, RG_O_B3 = 46, RG_O_B4 = RG_O_B3 + RG_MAXN3,
              RG_O_WO = RG_O_B4 + RG_MAXN4, RG_O_BO = RG_O_WO + RG_MAXN4, RG_O_W4 = RG_O_BO + 1;

template <int D>
__global__ __launch_bounds__(RG_BLOCK) void k_rn_input_grad(RnGradArgs a) {
  constexpr int DD = D * D, A2 = 2 * DD, W1 = D + 4, W2 = D + 2, PP = (DD + RG_BLOCK - 1) / RG_BLOCK,
                QA = (A2 + RG_BLOCK - 1) / RG_BLOCK, NW = RG_BLOCK / WAVE;
  __shared__ float tin[W1 * W1], a1p[W2 * W2], a2s[A2], dz2p[2 * W2 * W2], dz1p[W1 * W1];
  __shared__ float sw[RG_O_W4 + RG_MAXN4 * (RG_MAXN3 + D)];
  __shared__ float red[NW][RG_MAXN3], s_h3[RG_MAXN3], s_h4[RG_MAXN4], s_dz3[RG_MAXN3], s_dz4[RG_MAXN4], s_state[32], s_dzo;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  const int64_t n = blockIdx.x;
  const int slot = blockIdx.y;
  const int k = a.learner[slot];
  // ---- learner k's network (the rules of the forward's population launch, mfg_irl_population.h)
  int n3 = a.n3, n4 = a.n4;
  float keep = a.keep_prob;
  const float *c1w = a.c1w, *c1b = a.c1b, *c2w = a.c2w, *c2b = a.c2b, *w3 = a.w3, *b3 = a.b3, *w4 = a.w4, *b4 = a.b4, *wo = a.wo,
              *bo = a.bo;
  if (a.geom) {
    const mfg_rn_geom_t e = rn_geom_entry(a.geom, k);
    n3 = e.n3; n4 = e.n4; keep = e.keep_prob;
    c1w = a.c1w + a.s_net * k;
    c1b = c1w + 25;
    c2w = c1b + 1;
    c2b = c2w + 18;
    w3 = c2b + 2;
    b3 = w3 + (int64_t)n3 * A2;
    w4 = b3 + n3;
    b4 = w4 + n4 * (n3 + D);
    wo = b4 + n4;
    bo = wo + n4;
  } else if (a.per_learner_net && a.s_net > 0) {
    const int64_t o = a.s_net * k;
    c1w += o; c1b += o; c2w += o; c2b += o; w3 += o; b3 += o; w4 += o; b4 += o; wo += o; bo += o;
  } else if (a.per_learner_net) {
    c1w += 25 * (int64_t)k; c1b += k; c2w += 18 * (int64_t)k; c2b += 2 * (int64_t)k;
    w3 += (int64_t)n3 * A2 * k; b3 += (int64_t)n3 * k; w4 += (int64_t)n4 * (n3 + D) * k; b4 += (int64_t)n4 * k;
    wo += (int64_t)n4 * k; bo += k;
  }
  const int in4 = n3 + D;
  const float* state = a.state + a.s_state * k + n * D;
  const float* act = a.action + a.s_action * k + n * DD;
  // ---- every small weight to LDS; the images zeroed (their halos stay zero)
  if (tid < 25) sw[RG_O_C1W + tid] = c1w[tid];
  if (tid < 18) sw[RG_O_C2W + tid] = c2w[tid];
  if (tid < 2) sw[RG_O_C2B + tid] = c2b[tid];
  if (tid < n3) sw[RG_O_B3 + tid] = b3[tid];
  if (tid < n4) {
    sw[RG_O_B4 + tid] = b4[tid];
    sw[RG_O_WO + tid] = wo[tid];
  }
  if (tid == 0) {
    sw[RG_O_C1B] = c1b[0];
    sw[RG_O_BO] = bo[0];
  }
  for (int e = tid; e < n4 * in4; e += RG_BLOCK) sw[RG_O_W4 + e] = w4[e];
  if (tid < D) s_state[tid] = state[tid];
  for (int e = tid; e < W1 * W1; e += RG_BLOCK) {
    tin[e] = 0.0f;
    dz1p[e] = 0.0f;
  }
  for (int e = tid; e < W2 * W2; e += RG_BLOCK) a1p[e] = 0.0f;
  for (int e = tid; e < 2 * W2 * W2; e += RG_BLOCK) dz2p[e] = 0.0f;
  int py[PP], px[PP];
  float actv[PP];
#pragma unroll
  for (int q = 0; q < PP; ++q) {
    const int p = tid + q * RG_BLOCK;
    const int pc = p < DD ? p : 0;
    py[q] = pc / D;
    px[q] = pc - py[q] * D;
    actv[q] = p < DD ? act[p] : 0.0f;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PP; ++q)
    if (tid + q * RG_BLOCK < DD) tin[(py[q] + 2) * W1 + px[q] + 2] = actv[q];
  __syncthreads();
  // ---- forward: conv1 + ReLU
  float a1v[PP];
#pragma unroll
  for (int q = 0; q < PP; ++q) {
    a1v[q] = 0.0f;
    if (tid + q * RG_BLOCK < DD) {
      float s = sw[RG_O_C1B];
      const float* tp = tin + py[q] * W1 + px[q];
#pragma unroll
      for (int dy = 0; dy < 5; ++dy)
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) s = fmaf(tp[dy * W1 + dx], sw[RG_O_C1W + dy * 5 + dx], s);
      a1v[q] = fmaxf(s, 0.0f);
      a1p[(py[q] + 1) * W2 + px[q] + 1] = a1v[q];
    }
  }
  __syncthreads();
  // ---- conv2 + ReLU -> NHWC flat
#pragma unroll
  for (int q = 0; q < PP; ++q) {
    const int p = tid + q * RG_BLOCK;
    if (p < DD) {
      const float* tp = a1p + py[q] * W2 + px[q];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float s = sw[RG_O_C2B + c];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) s = fmaf(tp[dy * W2 + dx], sw[RG_O_C2W + c * 9 + dy * 3 + dx], s);
        a2s[p * 2 + c] = fmaxf(s, 0.0f);
      }
    }
  }
  __syncthreads();
  // ---- fc3: thread owns inputs i = tid + 256 q
  float a2v[QA];
#pragma unroll
  for (int q = 0; q < QA; ++q) {
    const int i = tid + q * RG_BLOCK;
    a2v[q] = i < A2 ? a2s[i] : 0.0f;
  }
  for (int u = 0; u < n3; ++u) {
    float s = 0.0f;
#pragma unroll
    for (int q = 0; q < QA; ++q) {
      const int i = tid + q * RG_BLOCK;
      if (i < A2) s = fmaf(a2v[q], w3[(int64_t)u * A2 + i], s);
    }
    s = wave_sum_f32_dpp(s);
    if (lane == 0) red[wv][u] = s;
  }
  __syncthreads();
  const bool drop = keep < 1.0f;
  const float inv_keep = drop ? 1.0f / keep : 1.0f;
  const uint64_t key = a.key[slot], ctr = a.sample_offset + (uint64_t)n;
  if (tid < n3) {
    float z = sw[RG_O_B3 + tid];
#pragma unroll
    for (int w = 0; w < NW; ++w) z += red[w][tid];
    float h = fmaxf(z, 0.0f);
    if (drop) {
      const u32x4 r = philox_elem(key, (uint32_t)tid, 3u, ctr, 0);
      h = (u01(r.x) <= keep) ? h * inv_keep : 0.0f;
    }
    s_h3[tid] = h;
  }
  __syncthreads();
  // ---- fc4 over [h3, state] (networks.py:72)
  if (tid < n4) {
    const float* w = sw + RG_O_W4 + tid * in4;
    float z = sw[RG_O_B4 + tid];
    for (int u = 0; u < n3; ++u) z = fmaf(s_h3[u], w[u], z);
    for (int j = 0; j < D; ++j) z = fmaf(s_state[j], w[n3 + j], z);
    float h = fmaxf(z, 0.0f);
    if (drop) {
      const u32x4 r = philox_elem(key, (uint32_t)tid, 4u, ctr, 0);
      h = (u01(r.x) <= keep) ? h * inv_keep : 0.0f;
    }
    s_h4[tid] = h;
  }
  __syncthreads();
  if (tid == 0) {
    float z = sw[RG_O_BO];
    for (int m = 0; m < n4; ++m) z = fmaf(s_h4[m], sw[RG_O_WO + m], z);
    const float r = tanhf(z);
    s_dzo = 1.0f - r * r;  // d r / d z_out
  }
  __syncthreads();
  // ---- backward to the inputs.  h > 0 <=> pre-activation > 0 and the unit kept; a kept unit carries 1 / keep_prob
  if (tid < n4) s_dz4[tid] = s_h4[tid] > 0.0f ? s_dzo * sw[RG_O_WO + tid] * inv_keep : 0.0f;
  __syncthreads();
  // fc4^T: column tid of fc4_w -- the first n3 are dh3, the other D the state's gradient
  if (tid < in4) {
    float s = 0.0f;
    for (int m = 0; m < n4; ++m) s = fmaf(s_dz4[m], sw[RG_O_W4 + m * in4 + tid], s);
    if (tid < n3) s_dz3[tid] = s_h3[tid] > 0.0f ? s * inv_keep : 0.0f;
    else a.gs[((int64_t)k * a.N + n) * D + (tid - n3)] = s;
  }
  __syncthreads();
  // fc3^T + ReLU: the derivative of the conv2 map, into the two padded images
#pragma unroll
  for (int q = 0; q < QA; ++q) {
    const int i = tid + q * RG_BLOCK;
    if (i < A2) {
      float s = 0.0f;
      for (int u = 0; u < n3; ++u) s = fmaf(s_dz3[u], w3[(int64_t)u * A2 + i], s);
      const int p = i >> 1, c = i & 1, y = p / D, x = p - y * D;
      dz2p[c * W2 * W2 + (y + 1) * W2 + x + 1] = a2v[q] > 0.0f ? s : 0.0f;
    }
  }
  __syncthreads();
  // transposed 3x3 convolution over both channels + ReLU of conv1: da1[y][x] = sum_c,dy,dx dz2[c][y - dy + 1][x - dx + 1] w[c][dy][dx]
#pragma unroll
  for (int q = 0; q < PP; ++q) {
    if (tid + q * RG_BLOCK < DD) {
      float s = 0.0f;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float* tp = dz2p + c * W2 * W2 + (py[q] + 2) * W2 + px[q] + 2;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) s = fmaf(tp[-dy * W2 - dx], sw[RG_O_C2W + c * 9 + dy * 3 + dx], s);
      }
      dz1p[(py[q] + 2) * W1 + px[q] + 2] = a1v[q] > 0.0f ? s : 0.0f;
    }
  }
  __syncthreads();
  // transposed 5x5 convolution: the action's gradient
#pragma unroll
  for (int q = 0; q < PP; ++q) {
    const int p = tid + q * RG_BLOCK;
    if (p < DD) {
      float s = 0.0f;
      const float* tp = dz1p + (py[q] + 4) * W1 + px[q] + 4;
#pragma unroll
      for (int dy = 0; dy < 5; ++dy)
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) s = fmaf(tp[-dy * W1 - dx], sw[RG_O_C1W + dy * 5 + dx], s);
      a.ga[((int64_t)k * a.N + n) * DD + p] = s;
    }
  }
}

// block (c, slot): element e of chunk c of the learner's samples, gradient and gradient x input, ascending n
__global__ __launch_bounds__(RG_BLOCK) void k_rn_grad_mean_partial(const float* __restrict__ gs, const float* __restrict__ ga,
                                                                   const float* __restrict__ state, const float* __restrict__ action,
                                                                   int64_t s_state, int64_t s_action, int64_t N, int d, int64_t rows,
                                                                   const int32_t* __restrict__ learner,
                                                                   double* __restrict__ partials) {
  const int c = blockIdx.x, chunks = gridDim.x, k = learner[blockIdx.y];
  const int dd = d * d, E = d + dd;
  const int64_t n0 = (int64_t)c * rows;
  const int64_t n1 = n0 + rows < N ? n0 + rows : N;  // (n0 >= N in the last chunks: an empty sum)
  double* out = partials + ((int64_t)k * chunks + c) * 2 * E;
  for (int e = threadIdx.x; e < E; e += RG_BLOCK) {
    const bool st = e < d;
    const int w = st ? d : dd, o = st ? e : e - d;
    const float* g = (st ? gs : ga) + (int64_t)k * N * w + o;
    const float* x = (st ? state + s_state * k : action + s_action * k) + o;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t n = n0; n < n1; ++n) {
      const double gv = (double)g[n * w], xv = (double)x[n * w];
      s0 += gv;
      s1 += gv * xv;  // (24-bit x 24-bit: exact in fp64)
    }
    out[e] = s0;
    out[E + e] = s1;
  }
}

// block (x, slot): thread t of the launch owns (q, e) = (t / E, t mod E) and adds the chunk totals in chunk order
__global__ __launch_bounds__(RG_BLOCK) void k_rn_grad_mean_fold(const double* __restrict__ partials, int chunks, int64_t N, int d,
                                                                const int32_t* __restrict__ learner, double* __restrict__ mean_state,
                                                                double* __restrict__ mean_action) {
  const int k = learner[blockIdx.y];
  const int dd = d * d, E = d + dd;
  const int t = blockIdx.x * RG_BLOCK + threadIdx.x;
  if (t >= 2 * E) return;
  const int q = t / E, e = t - q * E;
  const double* p = partials + (int64_t)k * chunks * 2 * E + (int64_t)q * E + e;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += p[(int64_t)c * 2 * E];
  s /= (double)N;
  if (e < d) {
    if (mean_state) mean_state[((int64_t)k * 2 + q) * d + e] = s;
  } else if (mean_action) {
    mean_action[((int64_t)k * 2 + q) * dd + (e - d)] = s;
  }
}

int rn_input_grad_check(const mfg_rn_input_grad_t& b, int K, int64_t N, int d) {
  REQUIRE(b.grad_state || b.grad_action || b.mean_state || b.mean_action, "reward input-gradient block: all four outputs are NULL");
  REQUIRE(b.K == K && b.N == N && b.d == d, "reward input-gradient block: set for another K, N or d than the call's");
  if (N > 0x7FFFFFFF) return fail(MFG_EUNSUPPORTED, "reward input-gradient block: N=%lld >= 2^31", (long long)N);
  const size_t need = rn_input_grad_layout(K, N, d).bytes;
  if (!b.workspace || b.workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "reward input-gradient workspace: need %lld bytes, have %lld", (long long)need,
                (long long)(b.workspace ? b.workspace_bytes : 0));
  return MFG_OK;
}

int launch_rn_input_grad(const mfg_rn_input_grad_t& b, const RnGradCall& c, hipStream_t st) {
  const int d = c.d, E = d + d * d;
  const RnGradLayout L = rn_input_grad_layout(c.K, c.N, d);
  char* ws = reinterpret_cast<char*>(b.workspace);
  float* samples = reinterpret_cast<float*>(ws + L.samples);
  double* partials = reinterpret_cast<double*>(ws + L.partials);
  RnGradArgs a{};
  a.state = c.state; a.action = c.action;
  a.s_state = c.s_state; a.s_action = c.s_action; a.N = c.N;
  a.c1w = c.net.conv1_w; a.c1b = c.net.conv1_b; a.c2w = c.net.conv2_w; a.c2b = c.net.conv2_b;
  a.w3 = c.net.fc3_w; a.b3 = c.net.fc3_b; a.w4 = c.net.fc4_w; a.b4 = c.net.fc4_b; a.wo = c.net.out_w; a.bo = c.net.out_b;
  a.n3 = c.net.n3; a.n4 = c.net.n4; a.keep_prob = c.net.keep_prob;
  a.per_learner_net = c.per_learner_net; a.s_net = c.s_net; a.geom = c.geom;
  a.key = c.key; a.learner = c.learner; a.sample_offset = c.sample_offset;
  a.gs = b.grad_state ? b.grad_state : samples;
  a.ga = b.grad_action ? b.grad_action : samples + (size_t)c.K * (size_t)c.N * (size_t)d;
  const dim3 g((unsigned)c.N, (unsigned)c.n);
  if (d == 21) hipLaunchKernelGGL(k_rn_input_grad<21>, g, dim3(RG_BLOCK), 0, st, a);
  else hipLaunchKernelGGL(k_rn_input_grad<15>, g, dim3(RG_BLOCK), 0, st, a);
  if (b.mean_state || b.mean_action) {
    const int chunks = action_mean_chunks(c.N);
    hipLaunchKernelGGL(k_rn_grad_mean_partial, dim3((unsigned)chunks, (unsigned)c.n), dim3(RG_BLOCK), 0, st, a.gs, a.ga, c.state,
                       c.action, c.s_state, c.s_action, c.N, d, action_mean_rows(c.N), c.learner, partials);
    hipLaunchKernelGGL(k_rn_grad_mean_fold, dim3((unsigned)((2 * E + RG_BLOCK - 1) / RG_BLOCK), (unsigned)c.n), dim3(RG_BLOCK), 0,
                       st, partials, chunks, c.N, d, c.learner, b.mean_state, b.mean_action);
  }
  return check_launch("rn_input_grad");
}

}  // namespace mfg

extern "C" size_t mfg_rn_input_grad_workspace_bytes(int K, int64_t N, int d) {
  if (K < 1 || N < 1 || d < 1) return 0;
  return mfg::rn_input_grad_layout(K, N, d).bytes;
}
