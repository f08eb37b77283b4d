#!/usr/bin/env python3
"""GPU: bootstrap replicates of the demonstrations (ops.demos_bootstrap) at the shape of tools/demos_probe.py -- U = 10^6 agents,
H = 16 hours, N = 24 days, C = 47, width = 20, d = 15, its contended ('zipf') and its uniform log -- at R = 4, 16, 64, 256.
Per R, event-timed on resident buffers, warmed, alternating rounds, medians:
  call    ops.demos_bootstrap (memsets, the counting pass, the finishing pass over R N days, the status pass)
  finish  the finishing pass alone (ops.demos_from_moves on the call's R N integer tables); call - finish bounds the counting
          pass with its memsets from above: its log bytes/s (the log is read once per block of four replicates, the first hour of a
          block of hours once more) and LDS atomics/s (one per agent, transition and replicate with w > 0 that is not absent at both hours:
          0.632 R times the unweighted events, which are sum present[h < H-1] + sum entered of the sample)
  (a)     R calls of ops.demos_from_logs on the same log: what a user could do before, and it does not even resample
  (b)     the same integer tables through torch: the log gathered by torch.randint indices per day and bincount per
          replicate, on --torch-replicates replicates, scaled to R
python tools/demos_bootstrap_probe.py [--rounds 5] [--agents 1000000] [--out profiles/demos_bootstrap.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from discrete_mean_field_game_amd import ops  # noqa: E402
from demos_probe import C, D, H, N, WIDTH, event_ms, make_log  # noqa: E402


def torch_replicate(topic, rank, g):
    """(b): counts and moves of ONE multinomial replicate with torch ops."""
    dev, U = topic.device, topic.shape[2]
    W1 = WIDTH + 1
    idx = torch.randint(U, (N, 1, U), device=dev, generator=g).expand(N, H, U)
    t = topic.long().gather(2, idx)
    seen = (t >= 0) & (t < C)
    cur = rank.long().gather(1, t.clamp(0, C - 1).view(N, H * U)).view(N, H, U)
    cur = torch.where(seen & (cur >= 0) & (cur < WIDTH), cur, torch.full_like(cur, WIDTH))
    row = torch.arange(N * H, device=dev).view(N, H, 1)
    counts = torch.bincount((row * W1 + cur).view(-1), minlength=N * H * W1)
    step = torch.arange(N * (H - 1), device=dev).view(N, H - 1, 1)
    moves = torch.bincount(((step * W1 + cur[:, :-1]) * W1 + cur[:, 1:]).view(-1), minlength=N * (H - 1) * W1 * W1)
    return counts, moves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--agents', type=int, default=1_000_000)
    ap.add_argument('--replicates', type=int, nargs='+', default=[4, 16, 64, 256])
    ap.add_argument('--torch-replicates', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev, U = torch.device('cuda:0'), a.agents
    gb = N * H * U * 4 / 1e9
    sample_bufs = {n: torch.empty(s, dtype=t, device=dev) for n, (s, t) in ops.demos_shapes(N, H, C, D, WIDTH).items()}
    sample_ws = torch.empty(ops.demos_workspace_bytes(N, H, C, WIDTH) // 8, dtype=torch.int64, device=dev)
    lines = ['demos_bootstrap_probe: %s, U=%d agents x H=%d hours x N=%d days (%.2f GB of int32), C=%d, width=%d, d=%d, unit agent_day, '
             '%d alternating rounds, ms (medians)' % (torch.cuda.get_device_name(0), U, H, N, gb, C, WIDTH, D, a.rounds)]
    med = lambda v: float(np.median(v))
    for kind in ('zipf', 'uniform'):
        topic = make_log(kind, U, dev, 7)
        plain = lambda: ops.demos_from_logs(topic, C, D, width=WIDTH, out=sample_bufs, workspace=sample_ws)
        plain()
        order = sample_bufs['order']
        rank = torch.empty_like(order).scatter_(1, order.long(), torch.arange(C, dtype=torch.int32, device=dev).expand(N, C).contiguous())
        events = int(sample_bufs['present'][:, :-1].sum().item() + sample_bufs['entered'].sum().item())
        g = torch.Generator(device=dev)
        g.manual_seed(3)
        torch_replicate(topic, rank, g)
        t_b = med([event_ms(lambda: [torch_replicate(topic, rank, g) for _ in range(a.torch_replicates)]) for _ in range(3)]) / a.torch_replicates
        lines.append('%s log: %d unweighted events (agent, transition) inside the recorded set; (b) torch, one replicate: %.1f ms'
                     % (kind, events, t_b))
        for Rn in a.replicates:
            bufs = {n: torch.empty(s, dtype=t, device=dev) for n, (s, t) in ops.demos_boot_shapes(Rn, N, H, D, WIDTH).items()}
            ws = torch.empty(ops.demos_bootstrap_workspace_bytes(Rn, N, H, C, WIDTH) // 8, dtype=torch.int64, device=dev)
            call = lambda: ops.demos_bootstrap(topic, rank, C, D, Rn, 11, width=WIDTH, out=bufs, workspace=ws)
            fin_out = {n: torch.empty((Rn * N,) + tuple(bufs[n].shape[2:]), dtype=bufs[n].dtype, device=dev)
                       for n in ops.DEMOS_MOVES_OUTPUTS}
            tables = (bufs['counts'].view(Rn * N, H, WIDTH), bufs['moves'].view(Rn * N, H - 1, WIDTH, WIDTH))
            finish = lambda: ops.demos_from_moves(tables[0], tables[1], D, out=fin_out)
            many = lambda: [plain() for _ in range(Rn)]
            for _ in range(2):
                call(), finish()
            plain()
            weighted = int(bufs['present'][:, :, 0].sum().item())
            t = {'call': [], 'finish': [], 'a': []}
            for _ in range(a.rounds):
                t['call'].append(event_ms(call))
                t['finish'].append(event_ms(finish))
                t['a'].append(event_ms(many))
            c, f, ta = med(t['call']), med(t['finish']), med(t['a'])
            count = max(c - f, 1e-6)
            tile, room = (WIDTH + 1) ** 2 * 4, 65536 - (C + 3) // 4 * 4     # boot_tiles of csrc/mfg_demos_boot.h
            rb = 4 if room // tile >= 4 else 1
            hb = min(H - 1, room // (rb * tile))
            # the log once per replicate block, the first hour of every further block of hours once more
            reads = -(-Rn // rb) * (H + -(-(H - 1) // hb) - 1) / H
            lines.append('R=%-4d call %9.3f   finish %8.3f   call - finish %9.3f: %.2f TB/s of log read (%.1f passes), %.1f G LDS atomics/s'
                         '   (a) R x from_logs %9.3f = %.2f x call   (b) R x torch %9.0f = %.0f x call   mean weight at hour 0: %.4f'
                         % (Rn, c, f, count, reads * gb / count, reads, 0.632 * Rn * events / count / 1e6, ta, ta / c, t_b * Rn,
                            t_b * Rn / c, weighted / (Rn * max(1, int(sample_bufs['present'][:, 0].sum().item())))))
            del bufs, ws, fin_out, tables
        del topic
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
