#!/usr/bin/env python3
"""GPU: demonstrations counted from a log, against the ways to do without the kernels.  The shape: U = 10^6 agents, H = 16
hours, N = 24 days, C = 47 categories, width = 20, d = 15 (a log of 1.5 GB), once with a Zipf-like popularity and agents that
mostly stay where they are (the contended case: most transitions land on a few diagonal cells) and once uniform.
  call    ops.demos_from_logs on resident buffers, event-timed; lds_update 'plain' (one LDS atomic per lane, the default)
          against 'combine' (lanes of a wave that hit the same cell are combined before the LDS atomic): the A/B
  (t)     the same outputs with torch on the same device: bincount for the first hour's popularity, a stable argsort for the
          ranking, a gather, and bincount over (day, hour, from, to) keys
  (n)     the NumPy restatement (tests/demos_ref.py) on the host, on --host-days days, scaled to N
Both device sides are warmed up; alternating rounds, medians.  The integer outputs of the three are compared exactly.  The log's
bytes over the call's time stand next to the 6.0-6.2 TB/s that the given-P kernel of this project reaches (the call reads the
log once, and hour 0 once more for the ranking).
python tools/demos_probe.py [--rounds 7] [--agents 1000000] [--host-days 2] [--out profiles/demos_from_logs.txt] [--kernels-only]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from discrete_mean_field_game_amd import ops  # noqa: E402
import demos_ref as R  # noqa: E402

H, N, C, WIDTH, D = 16, 24, 47, 20, 15


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def make_log(kind, U, dev, seed):
    """topic [N, H, U] int32 on the device.  'zipf': popularity ~ 1 / (c + 1)^1.2, an agent keeps its category with
    probability 0.8 and is absent with probability 0.02; 'uniform': every hour drawn afresh over the C categories."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    topic = torch.empty((N, H, U), dtype=torch.int32, device=dev)
    p = 1.0 / torch.arange(1, C + 1, dtype=torch.float64, device=dev) ** (1.2 if kind == 'zipf' else 0.0)
    cdf = torch.cumsum(p / p.sum(), 0).float()
    draw = lambda: torch.searchsorted(cdf, torch.rand(U, device=dev, generator=g)).clamp_(max=C - 1).int()
    for n in range(N):
        cur = draw()
        for h in range(H):
            if h and kind == 'zipf':
                cur = torch.where(torch.rand(U, device=dev, generator=g) < 0.8, cur, draw())
            elif h:
                cur = draw()
            topic[n, h] = cur
            if kind == 'zipf':
                topic[n, h][torch.rand(U, device=dev, generator=g) < 0.02] = -1
    return topic


def torch_side(topic):
    """(t): order, counts, moves, state and action of order='first_hour' with torch ops."""
    dev, U = topic.device, topic.shape[2]
    W1 = WIDTH + 1
    t = topic.long()
    seen = (t >= 0) & (t < C)
    day = torch.arange(N, device=dev).view(N, 1)
    raw0 = torch.bincount((day * C + t[:, 0].clamp(0, C - 1))[seen[:, 0]], minlength=N * C).view(N, C)
    order = torch.argsort(raw0, dim=1, descending=True, stable=True)
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(C, device=dev).expand(N, C))
    cur = rank.gather(1, t.clamp(0, C - 1).view(N, H * U)).view(N, H, U)
    cur = torch.where(seen & (cur < WIDTH), cur, torch.full_like(cur, WIDTH))
    row = torch.arange(N * H, device=dev).view(N, H, 1)
    counts = torch.bincount((row * W1 + cur).view(-1), minlength=N * H * W1).view(N, H, W1)[..., :WIDTH]
    step = torch.arange(N * (H - 1), device=dev).view(N, H - 1, 1)
    moves = torch.bincount(((step * W1 + cur[:, :-1]) * W1 + cur[:, 1:]).view(-1), minlength=N * (H - 1) * W1 * W1)
    moves = moves.view(N, H - 1, W1, W1)[:, :, :WIDTH, :WIDTH]
    state = (counts[..., :D].double() / counts.sum(-1, keepdim=True).double()).float()
    action = (moves[:, :, :D, :D].double() / moves.sum(-1, keepdim=True)[:, :, :D].double()).float()
    return {'order': order.int(), 'counts': counts.int(), 'moves': moves.int(), 'state': state, 'action': action}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--agents', type=int, default=1_000_000)
    ap.add_argument('--host-days', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernels-only', action='store_true', help='three device calls per form and nothing else: the run to put under rocprofv3')
    a = ap.parse_args()
    dev, U = torch.device('cuda:0'), a.agents
    shapes = ops.demos_shapes(N, H, C, D, WIDTH)
    bufs = {n: torch.empty(s, dtype=t, device=dev) for n, (s, t) in shapes.items()}
    ws = torch.empty(ops.demos_workspace_bytes(N, H, C, WIDTH) // 8, dtype=torch.int64, device=dev)
    gb = N * H * U * 4 / 1e9
    lines = ['demos_probe: %s, U=%d agents x H=%d hours x N=%d days (%.2f GB of int32), C=%d, width=%d, d=%d, order first_hour, '
             '%d alternating rounds, ms (medians; all rounds in brackets)' % (torch.cuda.get_device_name(0), U, H, N, gb, C, WIDTH, D, a.rounds)]
    for kind in ('zipf', 'uniform'):
        topic = make_log(kind, U, dev, 7)
        call = lambda form: ops.demos_from_logs(topic, C, D, width=WIDTH, out=bufs, workspace=ws, lds_update=form)
        for form in ('combine', 'plain'):
            for _ in range(3):
                call(form)
        torch.cuda.synchronize()
        if a.kernels_only:
            continue
        call('combine')
        other = {n: t.clone() for n, t in bufs.items()}
        call('plain')
        same_ab = all(torch.equal(other[n].view(torch.int32), bufs[n].view(torch.int32)) for n in bufs)
        del other
        ref = torch_side(topic)
        same_t = all(torch.equal(ref[n], bufs[n]) for n in ('order', 'counts', 'moves'))
        ok = torch.isfinite(ref['action'])
        same_t = same_t and torch.equal(ref['state'], bufs['state']) and torch.equal(ref['action'][ok], bufs['action'][ok])
        del ref
        t = {'combine': [], 'plain': [], 't': []}
        for _ in range(a.rounds):
            t['plain'].append(event_ms(lambda: call('plain')))
            t['combine'].append(event_ms(lambda: call('combine')))
            t['t'].append(event_ms(lambda: torch_side(topic)))
        days = topic[:a.host_days].cpu().numpy()
        t0 = time.perf_counter()
        want = R.from_logs(days, C, D, WIDTH)
        host_ms = 1e3 * (time.perf_counter() - t0) * N / a.host_days
        call('plain')
        same_n = R.differing({n: bufs[n][:a.host_days] for n in want}, want) == []
        med = {k: float(np.median(v)) for k, v in t.items()}
        fmt = lambda v: ' '.join('%.2f' % x for x in v)
        top = bufs['moves'].sum(0).sum(0).diagonal().sum().item() / max(1, bufs['moves'].sum().item())
        lines += ['%s log: %.0f %% of the transitions inside the recorded set lie on the diagonal' % (kind, 100 * top),
                  'call    ops.demos_from_logs, lds_update=plain (two memsets, four launches)      %8.3f [%s]   %.2f TB/s of log' % (
                      med['plain'], fmt(t['plain']), gb / med['plain']),
                  '        the same with lds_update=combine (A/B; identical outputs: %s)          %8.3f [%s]   %.2f TB/s of log' % (
                      same_ab, med['combine'], fmt(t['combine']), gb / med['combine']),
                  '(t)     the same outputs with torch (bincount, argsort, gather; equal: %s)     %8.3f [%s]   (t) / call = %.1f' % (
                      same_t, med['t'], fmt(t['t']), med['t'] / med['plain']),
                  '(n)     the NumPy restatement on the host, %d days scaled to %d (equal: %s)      %8.0f   (n) / call = %.0f' % (
                      a.host_days, N, same_n, host_ms, host_ms / med['plain'])]
        del topic
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
