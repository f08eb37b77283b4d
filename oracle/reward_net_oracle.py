"""NumPy restatement of the reference's reward network forward pass and IRL loss.  TEST INFRASTRUCTURE.

PARITY UNPINNED: ``networks.py`` / ``ac_irl.py:382-427`` need TensorFlow 1.x (``tf.contrib``), which cannot be
imported or installed here, and the reference holds no numeric test for the net.  This file therefore
follows the published semantics of the TF ops named in the reference (networks.py:46-81):
conv2d SAME stride 1 (cross-correlation, zero padding), ReLU, NHWC flatten, fully_connected, tanh;
``l1_l2_regularizer()`` = sum|W| + sum W^2 / 2 (scale_l1 = scale_l2 = 1); loss of ac_irl.py:390-413.
It is used to check the PyTorch module (weights shared), with dropout disabled.

Op semantics relied on (TensorFlow 1.x API documentation; none of it can be executed here):
  * tf.nn.conv2d / tf.contrib.layers.conv2d, NHWC, filter [kh, kw, in, out]: "computes ... output[b, i, j, k] =
    sum_{di, dj, q} input[b, strides[1]*i + di, strides[2]*j + dj, q] * filter[di, dj, q, k]" -- a CROSS-CORRELATION (no
    kernel flip); padding "SAME", stride 1, odd k: out size = in size, pad_total = k - 1 split as (k-1)/2 before and
    after, zeros.  => scipy.signal.correlate2d(x, w, mode='same') per (in, out) channel pair, summed over `in`
    (checked in tests/test_reward_net.py::test_oracle_conv_is_tf_same_cross_correlation with asymmetric kernels).
  * tf.reshape(conv2, [-1, f2*d*d]) of an NHWC tensor (networks.py:67): row-major over (h, w, c): index (h*d + w)*f2 + c.
  * tf.contrib.layers.fully_connected: activation(x . W + b), W [in, out]; weights_initializer = xavier_initializer()
    (uniform, limit sqrt(6 / (fan_in + fan_out))), biases_initializer = zeros.
  * tf.contrib.layers.l1_l2_regularizer(scale_l1=1.0, scale_l2=1.0) = l1_regularizer + l2_regularizer with
    l1 = scale_l1 * sum |W|, l2 = scale_l2 * tf.nn.l2_loss(W), and tf.nn.l2_loss(t) = sum(t ** 2) / 2.
  * tf.contrib.layers.dropout(x, keep_prob, is_training=True): tf.nn.dropout -- keeps each unit with probability
    keep_prob and scales the kept ones by 1 / keep_prob (inverted dropout); is_training defaults to True, so the
    reference applies it also when the net serves as the RL reward (ac_irl.py:683).
  * Checkpoint variables (tf.train.Saver, ac_irl.py:948): reward/<scope>/weights, reward/<scope>/biases with the layouts
    above; discrete_mean_field_game_amd.networks.RewardNet.load_tf_variables / tf_variables convert to / from them.
"""
import numpy as np


def conv2d_same(x, w, b):
    """x [N,H,W,Cin], w [kh,kw,Cin,Cout] (TF layout), stride 1, SAME zero padding."""
    N, H, W, Cin = x.shape
    kh, kw, _, Cout = w.shape
    ph, pw = kh // 2, kw // 2
    xp = np.zeros((N, H + 2 * ph, W + 2 * pw, Cin))
    xp[:, ph:ph + H, pw:pw + W] = x
    out = np.zeros((N, H, W, Cout))
    for u in range(kh):
        for v in range(kw):
            out += np.einsum('nhwc,co->nhwo', xp[:, u:u + H, v:v + W], w[u, v])
    return out + b


def dropout_masks(keep_prob, seed, sample_offset, N, n3, n4):
    """The dropout masks the HIP kernel draws (csrc/mfg_reward_net.hip): unit o of FC3 / FC4 of sample n is kept iff
    u01(Philox4x32-10(key = seed, counter = (o, 3 | 4, sample_offset + n, block 0)).x) <= keep_prob; kept units are scaled
    by 1 / keep_prob (tf.nn.dropout).  TF's own generator cannot be matched; what this pins is that the kernel evaluates
    the documented function of the documented bits, so a run WITH dropout (the reference's default reg='dropout_l1l2',
    active also when the net serves as the RL reward) can be replayed.  Returns (m3 [N,n3], m4 [N,n4]) of 0 / (1/keep)."""
    from oracle import philox_ref as PR
    n = np.arange(N, dtype=np.uint64) + np.uint64(sample_offset)
    inv = np.float32(1.0) / np.float32(keep_prob)
    out = []
    for units, step in ((n3, 3), (n4, 4)):
        o = np.arange(units, dtype=np.uint64)
        r = PR.philox_elem(int(seed), o[None, :], step, n[:, None], 0)[0]
        u = PR.u01(r)
        out.append(np.where(u <= np.float32(keep_prob), inv, np.float32(0.0)).astype(np.float64))
    return out[0], out[1]


def forward(params, state, action, dropout=None):
    """params: dict of TF-layout arrays conv1_w [5,5,1,1], conv1_b, conv2_w [3,3,1,2], conv2_b,
    fc3_w [2d^2,n3], fc3_b, fc4_w [n3+d,n4], fc4_b, out_w [n4,1], out_b.  Returns [N,1].
    dropout = (keep_prob, seed, sample_offset): apply the kernel's counter-based masks after fc3 and fc4."""
    N, d = state.shape
    x = action.reshape(N, d, d, 1).astype(np.float64)
    x = np.maximum(conv2d_same(x, params['conv1_w'], params['conv1_b']), 0)
    x = np.maximum(conv2d_same(x, params['conv2_w'], params['conv2_b']), 0)
    x = x.reshape(N, -1)                                            # NHWC flatten (networks.py:67)
    x = np.maximum(x.dot(params['fc3_w']) + params['fc3_b'], 0)
    m3 = m4 = None
    if dropout is not None:
        m3, m4 = dropout_masks(dropout[0], dropout[1], dropout[2], N, params['fc3_w'].shape[1], params['fc4_w'].shape[1])
        x = x * m3                                                   # networks.py:70
    x = np.concatenate([x, state.astype(np.float64)], axis=1)        # networks.py:72
    x = np.maximum(x.dot(params['fc4_w']) + params['fc4_b'], 0)
    if m4 is not None:
        x = x * m4                                                   # networks.py:75
    return np.tanh(x.dot(params['out_w']) + params['out_b'])


def l1_l2(params):
    return sum(np.abs(params[k]).sum() + 0.5 * (params[k] ** 2).sum() for k in ('fc3_w', 'fc4_w'))


def irl_loss(r_demo, r_gen, n_demo, n_traj, reg=0.0, steps=15):
    """n_traj == 0 (no generated trajectories): the second term is 0, as the kernel reports it; an empty r_demo gives first = 0."""
    first = -1.0 / n_demo * np.sum(r_demo)
    second = np.log(1.0 / n_traj * np.sum(np.exp(np.reshape(r_gen, (n_traj, steps)).sum(1)))) if n_traj else 0.0
    return first + second + reg, first, second


def params_from_torch(net):
    """Convert a networks.RewardNet state to the TF layouts used above."""
    g = lambda t: t.detach().cpu().double().numpy()
    return {
        'conv1_w': g(net.conv1.weight).transpose(2, 3, 1, 0), 'conv1_b': g(net.conv1.bias),
        'conv2_w': g(net.conv2.weight).transpose(2, 3, 1, 0), 'conv2_b': g(net.conv2.bias),
        'fc3_w': g(net.fc3.weight).T, 'fc3_b': g(net.fc3.bias),
        'fc4_w': g(net.fc4.weight).T, 'fc4_b': g(net.fc4.bias),
        'out_w': g(net.out.weight).T, 'out_b': g(net.out.bias),
    }


# ---------------------------------------------------------------------------------------------------------------------
# Training step (ac_irl.py:382-418 loss + tf.train.AdamOptimizer, :804-846 update_reward), fp64.  PARITY UNPINNED like the
# forward pass: this is the hand-derived gradient of the restated graph, checked against PyTorch autograd of
# networks.RewardNet and against central differences in tests/test_reward_net.py.
# ---------------------------------------------------------------------------------------------------------------------
def forward_cache(params, state, action, masks=None):
    """forward() that also returns what backward() needs.  masks = (m3 [N,n3], m4 [N,n4]) of 0 / (1/keep) or None."""
    N, d = state.shape
    x0 = action.reshape(N, d, d, 1).astype(np.float64)
    z1 = conv2d_same(x0, params['conv1_w'], params['conv1_b'])
    a1 = np.maximum(z1, 0)
    z2 = conv2d_same(a1, params['conv2_w'], params['conv2_b'])
    a2 = np.maximum(z2, 0)
    flat = a2.reshape(N, -1)
    z3 = flat.dot(params['fc3_w']) + params['fc3_b']
    h3 = np.maximum(z3, 0)
    if masks is not None:
        h3 = h3 * masks[0]
    in4 = np.concatenate([h3, state.astype(np.float64)], axis=1)
    z4 = in4.dot(params['fc4_w']) + params['fc4_b']
    h4 = np.maximum(z4, 0)
    if masks is not None:
        h4 = h4 * masks[1]
    r = np.tanh(h4.dot(params['out_w']) + params['out_b'])
    # smallest |pre-activation| of a ReLU, relative to the magnitude of the terms it sums: an fp32 evaluation may land on the
    # other side of a kink this close to zero, and the gradient then differs by that unit's whole contribution -- a dense
    # unit carries a sample's whole share of the fc gradients, a conv pixel ~1e-4 of a conv-weight gradient (one of ~8 000
    # pixel terms).  The randomised soak (tools/rn_train_soak.py) skips such draws.
    m3 = np.abs(flat).dot(np.abs(params['fc3_w'])) + np.abs(params['fc3_b'])
    m4 = np.abs(in4).dot(np.abs(params['fc4_w'])) + np.abs(params['fc4_b'])
    m1 = conv2d_same(np.abs(x0), np.abs(params['conv1_w']), np.abs(params['conv1_b']))
    m2 = conv2d_same(np.abs(a1), np.abs(params['conv2_w']), np.abs(params['conv2_b']))
    kink = min(float((np.abs(z) / np.maximum(m, 1e-300)).min()) for z, m in ((z1, m1), (z2, m2), (z3, m3), (z4, m4)))
    return r, dict(x0=x0, a1=a1, a2=a2, flat=flat, h3=h3, in4=in4, h4=h4, r=r, masks=masks, kink=kink)


def _conv_backward(x, w, dz):
    """Gradients of z = conv2d_same(x, w, b) given dz [N,H,W,Cout]: (dx, dw, db)."""
    N, H, W, Cin = x.shape
    kh, kw, _, Cout = w.shape
    ph, pw = kh // 2, kw // 2
    xp = np.zeros((N, H + 2 * ph, W + 2 * pw, Cin))
    xp[:, ph:ph + H, pw:pw + W] = x
    dxp = np.zeros_like(xp)
    dw = np.zeros_like(w, dtype=np.float64)
    for u in range(kh):
        for v in range(kw):
            dw[u, v] = np.einsum('nhwc,nhwo->co', xp[:, u:u + H, v:v + W], dz)
            dxp[:, u:u + H, v:v + W] += np.einsum('nhwo,co->nhwc', dz, w[u, v])
    return dxp[:, ph:ph + H, pw:pw + W], dw, dz.sum(axis=(0, 1, 2))


def backward(params, cache, dr):
    """d (sum_n dr_n r_n) / d params for dr [N,1]; TF layouts like `params`."""
    m = cache['masks']
    dzo = dr * (1.0 - cache['r'] ** 2)
    g = {'out_w': cache['h4'].T.dot(dzo), 'out_b': dzo.sum(0)}
    dh4 = dzo.dot(params['out_w'].T)
    dz4 = dh4 * (cache['h4'] > 0) * (m[1] if m is not None else 1.0)
    g['fc4_w'] = cache['in4'].T.dot(dz4)
    g['fc4_b'] = dz4.sum(0)
    n3 = params['fc3_w'].shape[1]
    dh3 = dz4.dot(params['fc4_w'].T)[:, :n3]
    dz3 = dh3 * (cache['h3'] > 0) * (m[0] if m is not None else 1.0)
    g['fc3_w'] = cache['flat'].T.dot(dz3)
    g['fc3_b'] = dz3.sum(0)
    da2 = dz3.dot(params['fc3_w'].T).reshape(cache['a2'].shape)
    dz2 = da2 * (cache['a2'] > 0)
    da1, g['conv2_w'], g['conv2_b'] = _conv_backward(cache['a1'], params['conv2_w'], dz2)
    dz1 = da1 * (cache['a1'] > 0)
    _, g['conv1_w'], g['conv1_b'] = _conv_backward(cache['x0'], params['conv1_w'], dz1)
    return g


def irl_loss_and_grad(params, demo_state, demo_action, gen_state, gen_action, n_demo_div, n_traj, l1l2=False, steps=15,
                      masks=None, dr=None):
    """Loss of ac_irl.py:390-413 and its gradient for one update_reward batch.  masks: (m3, m4) over the concatenated batch
    (demonstrations first) or None.  Either half may be empty (arrays of shape [0, d] / [0, d, d]; n_traj == 0: second term 0,
    no generated coefficients).  dr [N,1]: coefficients dL/dr_n computed elsewhere (coefficients_from_rewards) that replace the
    ones derived from this function's own rewards in the backward pass; the loss terms stay this function's own.
    Returns ((loss, first, second, reg), grads dict, rewards [N,1])."""
    nd = demo_state.shape[0]
    state = np.concatenate([demo_state, gen_state], 0)
    action = np.concatenate([demo_action, gen_action], 0)
    r, cache = forward_cache(params, state, action, masks)
    reg = l1_l2(params) if l1l2 else 0.0
    loss, first, second = irl_loss(r[:nd], r[nd:], n_demo_div, n_traj, reg, steps)
    if dr is None:
        dr = _coefficients(r, nd, n_traj, steps, -1.0 / n_demo_div)
    g = backward(params, cache, np.asarray(dr, dtype=np.float64).reshape(-1, 1))
    if l1l2:
        for k in ('fc3_w', 'fc4_w'):
            g[k] = g[k] + np.sign(params[k]) + params[k]
    return (loss, first, second, reg), g, r


def _coefficients(r, nd, n_traj, steps, demo_coefficient):
    """dL/dr_n [N,1] from fp64 rewards r [N,1]: demo_coefficient for the nd demonstration transitions, the soft-max over the
    generated trajectories' reward sums for theirs."""
    if n_traj == 0:
        return np.full((nd, 1), demo_coefficient)
    S = r[nd:].reshape(n_traj, steps).sum(1)
    soft = np.exp(S - S.max())
    soft = soft / soft.sum()
    return np.concatenate([np.full((nd, 1), demo_coefficient), np.repeat(soft, steps)[:, None]], 0)


# ---------------------------------------------------------------------------------------------------------------------
# The coefficient phase of the combine kernel (csrc/mfg_reward_train.hip, rn_train_combine_body), restated from the fp32
# rewards that launch 1 left in the workspace.  Everything the kernel does between those rewards and the coefficients c_n is
# a handful of fp32 operations; the budgets below are first order in
#     U = 2^-24, the unit roundoff of fp32: one correctly rounded +, -, *, / loses at most U of its result
#     (the library is built without fast-math: fp32 division is correctly rounded; additions are not reassociated);
#     expf, logf: 1 ulp = 2 U of the result (HIP math API, "maximum ULP error" of expf / logf on the device).
#
# S_j.  `for t: sacc += s_cn[(nd + j) T + t]`: an fp32 running sum in step order, one add per step, nothing to fuse.  NumPy
#   float32 additions are the same IEEE operation: S32 below IS the kernel's S_j, bit for bit, given the kernel's rewards.
#
# c_j = e_j / z, e_j = expf(S_j - mx), mx = max_j S_j (fmaxf / shuffles: exact), z = DPP sum of the 64 lanes' e_j.
#   d_j = fl(S_j - mx)              |d_j - (S_j - mx)| <= U |S_j - mx|;   exp turns it into a RELATIVE error |S_j - mx| U
#   e_j = expf(d_j)                 2 U
#   z   = 6 tree levels of adds     non-negative terms (lanes >= ng add an exact 0): 6 U of z, besides the e_j's own errors,
#                                   which z inherits as a weighted mean  sum_j c_j (|S_j - mx| + 2) U  <=  max_j of it
#   e_j / z                         U
#   With e_i (1 + delta_i), |delta_i| <= (|S_i - mx| + 2) U, the tree returns z (1 + sum_i c_i delta_i + 6 U): z inherits the
#   e_i's errors as their c-weighted mean, at most (zbar + 2) U with zbar = sum_i c_i |S_i - mx| (small: the weight sits where
#   |S_i - mx| ~ 0).  Together
#       eps_j = (|S_j - mx| + 2  +  zbar + 2 + 6  +  1  +  1) U = (|S_j - mx| + zbar + C0) U,   C0 = 12,
#   the last 1 covering every second-order term ((|d| + 11)^2 U^2 < U while |d| < 4000).  The bound is claimed while e_j is
#   a normal fp32 number, S_j - mx > -87; below that expf flushes and eps_j is reported as inf (such a trajectory adds at
#   most e^-87 to z's relative error, nothing next to U).
#
# second = mx + logf(z / ng):   z / ng carries z's relative error (zbar + 2 + 6) U and the division's U; logf turns a relative
#   error of its argument into an absolute one and adds 2 U |log(z / ng)| of its own; the final addition rounds once:
#   second_bound = (zbar + 2 + 6 + 1 + 2 |ln(z / ng)| + 1) U + U |second|.          (ng = 0: second = 0 exactly, bound 0)
#
# first = -fl(1 / divisor) * sd:   sd is the demonstration rewards summed by one wave: lane l adds n = l, l + 64, ... in
#   order (k = ceil(nd T / 64) terms, k - 1 additions), then the 6-level tree; every addition loses at most U of a partial sum
#   that is at most sum |r_demo|: (k - 1 + 6) U sum |r_demo|.  fl(1 / divisor) and the product round once each:
#   first_bound = (k + 5 + 2 + 1) U sum |r_demo| / divisor                           (nd = 0: first = -0 exactly, bound 0)
#
# loss = fl(fl(first + second) + reg): two more roundings, U |first + second| + U |loss|, on top of the terms' own bounds.
# ---------------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24
C0_SOFTMAX = 12.0
EXPF_NORMAL_MIN = -87.0


def coefficients_from_rewards(r, n_demo, n_gen, steps, demo_divisor):
    """The combine kernel's coefficient phase on fp32 rewards r [N] (N = (n_demo + n_gen) steps, demonstrations first).
    Returns a dict:
      S32 [n_gen] float32   the per-trajectory sums exactly as the kernel forms them (fp32 running sum in step order)
      c [N,1] float64       dL/dr_n: -1/demo_divisor (demonstrations), soft-max of S32 (generated); c_traj [n_demo + n_gen]
      first, second         the loss terms in fp64 from the same inputs
      eps [n_gen]           relative bound on the kernel's fp32 soft-max weight (derivation above); inf where expf flushes
      first_bound, second_bound   absolute bounds on the kernel's stats[1], stats[2];  loss_rounding(reg): the two final adds"""
    r32 = np.asarray(r, dtype=np.float32).reshape(-1)
    nd_t = n_demo * steps
    if r32.size != (n_demo + n_gen) * steps:
        raise ValueError('coefficients_from_rewards: %d rewards for (%d + %d) x %d' % (r32.size, n_demo, n_gen, steps))
    S32 = np.zeros(n_gen, dtype=np.float32)
    rg = r32[nd_t:].reshape(n_gen, steps)
    for t in range(steps):
        S32 = (S32 + rg[:, t]).astype(np.float32)         # one fp32 add per step
    r_demo = r32[:nd_t].astype(np.float64)
    sum_abs = float(np.abs(r_demo).sum())
    first = -1.0 / demo_divisor * float(r_demo.sum())
    k = -(-nd_t // 64)
    first_bound = (k + 8) * U32 * sum_abs / demo_divisor if n_demo else 0.0
    if n_gen:
        S = S32.astype(np.float64)
        dj = S - S.max()
        e = np.exp(dj)
        z = e.sum()
        soft = e / z
        zbar = float((soft * np.abs(dj)).sum())
        eps = np.where(dj > EXPF_NORMAL_MIN, (np.abs(dj) + zbar + C0_SOFTMAX) * U32, np.inf)
        second = float(S.max() + np.log(z / n_gen))
        second_bound = (zbar + 10.0 + 2.0 * abs(np.log(z / n_gen))) * U32 + U32 * abs(second)
    else:
        soft, eps, second, second_bound = np.zeros(0), np.zeros(0), 0.0, 0.0
    c_traj = np.concatenate([np.full(n_demo, -1.0 / demo_divisor), soft])
    return dict(S32=S32, c=np.repeat(c_traj, steps)[:, None], c_traj=c_traj, first=first, second=second, eps=eps,
                first_bound=first_bound, second_bound=second_bound,
                loss_rounding=lambda reg: U32 * (abs(first + second) + abs(first + second + reg)))


def grad_scale(prm, ds, da, gs, ga, n_div, n_traj, masks, l1l2, steps=None, coeff=None, gen_only=False, cache=None):
    """Per-parameter magnitude of the terms the batch gradient sums: the gradient with |dL/dr_n| as sample weights.  The
    demonstration (-) and generated (+) halves cancel to a small net value (e.g. out_b: 15 - 15 -> 0.03), and an fp32
    result can only be accurate relative to what was summed; the GPU tests' tolerances are 1e-5 of max(|net|, this scale).
    steps: transitions per trajectory (default: the generated half split evenly over n_traj); coeff [N] / [N,1]: given
    coefficients dL/dr_n instead of the ones derived from the oracle's own rewards; gen_only: the generated half alone (the
    demonstrations get weight 0); cache: forward_cache of this batch, if the caller has it.  Flat kernel order."""
    nd = ds.shape[0]
    if cache is None:
        state, action = np.concatenate([ds, gs], 0), np.concatenate([da, ga], 0)
        _, cache = forward_cache(prm, state, action, masks)
    r = cache['r']
    if coeff is not None:
        dr = np.abs(np.asarray(coeff, dtype=np.float64).reshape(-1, 1))
    elif n_traj:
        S = r[nd:].reshape(n_traj, -1 if steps is None else steps).sum(1)
        soft = np.exp(S - S.max()); soft /= soft.sum()
        dr = np.concatenate([np.full((nd, 1), 1.0 / n_div), np.repeat(soft, r[nd:].shape[0] // n_traj)[:, None]], 0)
    else:
        dr = np.full((nd, 1), 1.0 / n_div)
    if gen_only:
        dr = dr.copy()
        dr[:nd] = 0.0
    g = backward(prm, dict(cache), dr)
    return np.abs(flatten_like_kernel(g))


def adam_tf(p, g, m, v, step, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """tf.train.AdamOptimizer (ac_irl.py:417): lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t); m, v exponential averages;
    p -= lr_t m / (sqrt(v) + eps).  Returns (p, m, v)."""
    lr_t = lr * np.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


FLAT_ORDER = ('conv1_w', 'conv1_b', 'conv2_w', 'conv2_b', 'fc3_w', 'fc3_b', 'fc4_w', 'fc4_b', 'out_w', 'out_b')


def flatten_like_kernel(tf_arrays):
    """TF-layout dict -> the flat parameter order of mfg_reward_net_train_step (PyTorch layouts: conv OIHW, dense [out, in])."""
    out = []
    for k in FLAT_ORDER:
        a = np.asarray(tf_arrays[k], dtype=np.float64)
        if a.ndim == 4:
            a = a.transpose(3, 2, 0, 1)
        elif a.ndim == 2:
            a = a.T
        out.append(a.reshape(-1))
    return np.concatenate(out)
