#!/usr/bin/env python3
"""GPU: the Dirichlet-multinomial likelihood (ops.moves_loglik_pop) at the grid-search shape -- K = 1 000 policies, N = 24 days,
H = 16 hours, d = 21 and 15 -- on synthetic demonstrations (--agents agents a day, 3 000 by default so that most cells hold a handful: a topic keeps 80 %, the rest
move by popularity).  Per d, event-timed on resident buffers, warmed, alternating rounds, medians:
  call     ops.moves_loglik_pop, value and gradient (the three launches); `value` the same without the gradient
  torch    the same table from torch.lgamma / torch.special.digamma expressions over [K, N, H-1, d, d] on the same device: the
           plain differences lgamma(a + m) - lgamma(a) and digamma(a + m) - digamma(a)
  errors   of both against the restatement (tests/moves_loglik_ref.py) on --sample policies x 6 transitions, worst ratio to
           the tests' bound (1e-10 of the condition sums S and G)
  by path  the call on three count tables of the same shape that take one path each: empty, m = 3 in every cell, m = 40
  fit      likelihood.fit of 200 steps at K = 64 starts (host clock, ends in the read-back): kernel calls plus the torch update
python tools/moves_loglik_probe.py [--rounds 7] [--out profiles/moves_loglik.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from discrete_mean_field_game_amd import demos, likelihood, ops  # noqa: E402
from discrete_mean_field_game_amd.population import grid_points  # noqa: E402
import moves_loglik_ref as R  # noqa: E402

N, H, K_GRID, K_FIT, FIT_STEPS = 24, 16, 1000, 64, 200


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def make_demos(d, agents, dev, seed=3):
    """A Demonstrations of N days: counts from a popularity vector, moves row i multinomial(n_i, 0.8 e_i + 0.2 popularity)."""
    rs = np.random.RandomState(seed)
    counts = np.zeros((N, H, d), np.int32)
    moves = np.zeros((N, H - 1, d, d), np.int32)
    for n in range(N):
        pop = rs.dirichlet(np.full(d, 0.7))
        c = rs.multinomial(agents, pop)
        for h in range(H - 1):
            counts[n, h] = c
            for i in range(d):
                moves[n, h, i] = rs.multinomial(c[i], 0.8 * np.eye(d)[i] + 0.2 * pop)
            c = moves[n, h].sum(0)
        counts[n, H - 1] = c
    return demos.from_moves(counts, moves, d, device=dev)


def torch_table(state, moves, th, sh, al):
    """ll [K, N, H-1] and grad [K, N, H-1, 3] by the textbook expressions."""
    pi = state[:, :H - 1].double()
    m = moves.double()[None]
    x = pi[None, :, :, None, :] - pi[None, :, :, :, None] - sh.view(-1, 1, 1, 1, 1)
    z = th.view(-1, 1, 1, 1, 1) * x
    e = torch.exp(z)
    a = al.view(-1, 1, 1, 1, 1) * torch.log1p(e)
    sg = e / (1.0 + e)
    A, n = a.sum(-1), m.sum(-1)
    ll = (torch.lgamma(n + 1) - torch.lgamma(m + 1).sum(-1) + (torch.lgamma(a + m) - torch.lgamma(a)).sum(-1)
          - (torch.lgamma(A + n) - torch.lgamma(A))).sum(-1)
    Dj = torch.special.digamma(a + m) - torch.special.digamma(a)
    DA = torch.special.digamma(A + n) - torch.special.digamma(A)
    grads = []
    for da in (al.view(-1, 1, 1, 1, 1) * sg * x, -(al * th).view(-1, 1, 1, 1, 1) * sg, a):
        grads.append(((Dj * da).sum(-1) - DA * da.sum(-1)).sum(-1))
    return ll, torch.stack(grads, -1)


def worst_ratio(ll, grad, dm, par, sample):
    """Worst |value - restatement| / (1e-10 S) and |gradient - restatement| / (1e-10 G) over `sample` policies x 6 transitions."""
    rs = np.random.RandomState(1)
    w = [0.0, 0.0]
    for k in rs.choice(len(par), sample, replace=False):
        for n, h in zip(rs.randint(0, N, 6), rs.randint(0, H - 1, 6)):
            ref = R.transition(dm.state[n, h], dm.moves[n, h, :dm.d, :dm.d], *par[k])
            w[0] = max(w[0], abs(ll[k, n, h] - ref[0]) / (R.BOUND * ref[2]))
            w[1] = max(w[1], float(np.max(np.abs(grad[k, n, h] - ref[1]) / (R.BOUND * ref[3]))))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--agents', type=int, default=3000)
    ap.add_argument('--sample', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    med = lambda v: float(np.median(v))
    points = grid_points(np.linspace(7.0, 10.6, 10), np.linspace(0.0, 0.18, 10), np.geomspace(3e3, 3e4, 10))
    par = np.array(points)
    assert len(points) == K_GRID
    th, sh, al = (torch.as_tensor(par[:, c].copy(), device=dev) for c in range(3))
    lines = ['moves_loglik_probe: %s, K=%d policies x N=%d days x H=%d hours, %d agents a day, %d alternating rounds, ms (medians)'
             % (torch.cuda.get_device_name(0), K_GRID, N, H, a.agents, a.rounds)]
    for d in (21, 15):
        dm = make_demos(d, a.agents, dev)
        state, moves = torch.as_tensor(dm.state, device=dev), torch.as_tensor(dm.moves, device=dev)
        out = {n: torch.empty(s, dtype=t, device=dev) for n, (s, t) in ops.moves_loglik_shapes(K_GRID, N, H).items()}
        ws = torch.empty(ops.moves_loglik_workspace_bytes(K_GRID, 1, N, H, d) // 8, dtype=torch.int64, device=dev)
        call = lambda: ops.moves_loglik_pop(state, moves, th, sh, al, d, out=out, workspace=ws)
        value = lambda: ops.moves_loglik_pop(state, moves, th, sh, al, d, grad=False, out=out, workspace=ws)
        plain = lambda: torch_table(state, moves, th, sh, al)
        for _ in range(2):
            call(), value(), plain()
        t = {'call': [], 'value': [], 'torch': []}
        for _ in range(a.rounds):
            t['call'].append(event_ms(call))
            t['value'].append(event_ms(value))
            t['torch'].append(event_ms(plain))
        call()
        ll_t, grad_t = plain()
        assert int(out['status'].count_nonzero().item()) == 0
        mine = worst_ratio(out['ll'].cpu().numpy(), out['grad'].cpu().numpy(), dm, par, a.sample)
        theirs = worst_ratio(ll_t.cpu().numpy(), grad_t.cpu().numpy(), dm, par, a.sample)
        del ll_t, grad_t
        torch.cuda.empty_cache()
        cells = K_GRID * N * (H - 1) * d * d
        c, v, p = med(t['call']), med(t['value']), med(t['torch'])
        lines.append('d=%-2d call %8.3f (min %.3f max %.3f)  value only %8.3f  = %.1f G cells/s   torch %9.3f (min %.3f max %.3f) = %.1f x call'
                     % (d, c, min(t['call']), max(t['call']), v, cells / c / 1e6, p, min(t['torch']), max(t['torch']), p / c))
        lines.append('      worst error / bound on %d policies x 6 transitions: kernel value %.3g gradient %.3g; torch value %.3g gradient %.3g'
                     % (a.sample, mine[0], mine[1], theirs[0], theirs[1]))
        # what the cell pass spends its time on: the same call on count tables that take one path each
        parts = []
        for label, fill in (('no agents (softplus only)', 0), ('m = 3 everywhere (finite sums)', 3), ('m = 40 everywhere (series)', 40)):
            filled = torch.full_like(moves, fill)
            one = lambda: ops.moves_loglik_pop(state, filled, th, sh, al, d, out=out, workspace=ws)
            one()
            parts.append('%s %.3f' % (label, med([event_ms(one) for _ in range(a.rounds)])))
        lines.append('      by path: ' + ', '.join(parts))
        start = par[np.random.RandomState(2).choice(K_GRID, K_FIT, replace=False)]
        likelihood.fit(dm, start[:, 0], start[:, 1], start[:, 2], steps=3, device=dev)
        fits = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit = likelihood.fit(dm, start[:, 0], start[:, 1], start[:, 2], steps=FIT_STEPS, device=dev)
            fits.append((time.perf_counter() - t0) * 1e3)
        lines.append('      fit: %d steps, K=%d starts: %.1f ms (min %.1f max %.1f), %d frozen; mean log-likelihood %.6g -> %.6g; '
                     'median estimate theta %.4f shift %.4f alpha_scale %.1f'
                     % (FIT_STEPS, K_FIT, med(fits), min(fits), max(fits), int((fit.status != 0).sum()), np.nanmean(fit.trace[0]),
                        np.nanmean(fit.best_ll), *np.median(fit.best_params, 0)))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
