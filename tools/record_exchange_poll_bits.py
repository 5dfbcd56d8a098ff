#!/usr/bin/env python3
"""Records the fixture of tests/test_gpu_vamp_exchange_poll.py (tests/golden/exchange_poll_bits.part<k>.npz):
VAMP forwards over many workgroups whose batch is a tiling of ROWS stored trials.

  python tools/record_exchange_poll_bits.py [--out DIR]

Nt = 256, Na = 8, Nr = 512, 16-QAM on the channel that tests/golden/exchange_chain_bits.part*.npz
stores ('shared/U', 's', 'Vh', 'SNR': not stored again).  ROWS = 40 trials (x, sym, idx, y) are drawn
once; a batch of B trials takes trial b % ROWS as its row b, for B = 1040, 2064 and 4096: 65, 129 and
256 workgroups of 16 trials, so that a lane of the exchange's gather holds two, three and four granule
pairs, and B N is a power of two at B = 4096 only.  An output row of the engine depends on its own y
and on the batch scalars alone, so every tile of a batch equals its first ROWS rows bit for bit: the
script asserts that on the commit it runs on, and that the reuse forward on the same y equals the
building forward, and stores per batch the first ROWS rows of r, xmmse and var once, with T,
nan_state and the 13 counters of both forwards.

Public API only (Config, Channel, Data, VAMP, amp_native.prepare_counts, through
record_forward_bits), so the same script runs on any commit: a change that must leave the engine's
results bit-identical is checked against a fixture recorded on its parent.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'amp-sparc-spatialmodulation_amd'))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))

import numpy as np  # noqa: E402
import torch        # noqa: E402

import record_forward_bits as rec  # noqa: E402

STEM = 'exchange_poll_bits'
CHANNEL_STEM = 'exchange_chain_bits'
NT, NA, NR, ALPHABET = 256, 8, 512, '16QAM'
ROWS = 40
BATCHES = (1040, 2064, 4096)
FIELDS = ('r', 'xmmse', 'var')


def load_parts(golden, stem):
    """{name: array} of a fixture's parts, row blocks ('name@i') joined."""
    raw, k = {}, 0
    while os.path.exists(os.path.join(golden, f'{stem}.part{k}.npz')):
        z = np.load(os.path.join(golden, f'{stem}.part{k}.npz'))
        raw.update({n: z[n] for n in z.files})
        k += 1
    assert k, f'no parts of {stem} in {golden}'
    blocks = {}
    for n, a in raw.items():
        base, _, i = n.partition('@')
        blocks.setdefault(base, []).append((int(i or 0), a))
    return {base: (bl[0][1] if len(bl) == 1 else np.concatenate([a for _, a in sorted(bl, key=lambda p: p[0])], axis=0))
            for base, bl in blocks.items()}


def channel(golden):
    """The stored channel: U, s, Vh as host tensors and its SNR."""
    fx = load_parts(golden, CHANNEL_STEM)
    return dict(U=torch.from_numpy(fx['shared/U']), s=torch.from_numpy(fx['shared/s']), Vh=torch.from_numpy(fx['shared/Vh']),
                SNR=float(fx['shared/SNR'][0]))


def tiled(ep, B):
    """The batch of B trials whose row b is stored trial b % ROWS (x, sym, idx, y as Data and Channel give them)."""
    rows = np.arange(B) % ROWS
    nz = NA                                                  # non-zero entries per trial (no 16-QAM point is 0)
    idx = np.asarray(ep['idx']).reshape(ROWS, nz) - np.arange(ROWS)[:, None] * NT
    return dict(x=ep['x'][rows].contiguous(), y=ep['y'][rows].contiguous(),
                sym=np.ascontiguousarray(np.asarray(ep['sym']).reshape(ROWS, nz)[rows].reshape(-1)),
                idx=np.ascontiguousarray((idx[rows] + np.arange(B)[:, None] * NT).reshape(-1)))


def run_batch(ch, ep, B, device):
    """A building forward and a reuse forward on the same tiled batch: [(made, outputs)] * 2."""
    from vamp import VAMP
    det = VAMP(rec.config(NT, NA, NR, B, ALPHABET, device='cuda'))
    chan = tuple(ch[k].to(device).contiguous() for k in ('U', 's', 'Vh'))
    big = tiled(ep, B)
    return [rec.forward(det, chan, ch['SNR'], big, device) for _ in range(2)]


def tiles_differ(a):
    """Rows of a [B, ...] that differ from row b % ROWS (bitwise)."""
    a = np.ascontiguousarray(a)
    v = a.view(np.uint8).reshape(a.shape[0], -1)
    return np.flatnonzero((v != v[np.arange(a.shape[0]) % ROWS]).any(axis=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    ap.add_argument('--golden', default=os.path.join(REPO, 'tests', 'golden'), help='where the stored channel lies')
    args = ap.parse_args()
    device = torch.device('cuda', 0)
    ch = channel(args.golden)
    A = (ch['U'] * ch['s'].to(ch['U'].dtype)) @ ch['Vh']
    inp = rec.make_inputs((NT, NA, NR, ROWS, ALPHABET), shared=dict(A=A, U=ch['U'], s=ch['s'], Vh=ch['Vh'], SNR=ch['SNR']))
    ep = inp['eps'][0]
    flat = {k: rec.as_np(ep[k]) for k in ('x', 'sym', 'idx', 'y')}
    for B in BATCHES:
        res = run_batch(ch, ep, B, device)
        (m0, o0), (m1, o1) = res
        assert (m0, m1) == ((1, 0), (0, 1)), (m0, m1)
        for k in FIELDS:
            assert tiles_differ(o0[k]).size == 0 and tiles_differ(o1[k]).size == 0, (B, k)
            assert np.array_equal(o0[k].view(np.uint8), o1[k].view(np.uint8)), (B, k, 'reuse != building')
            flat[f'B{B}/{k}'] = o0[k][:ROWS].copy()
        for i, o in enumerate((o0, o1)):
            for k in ('T', 'nan_state', 'counts'):
                flat[f'B{B}/f{i}_{k}'] = o[k]
        print(f'B = {B}: T {int(o0["T"][0])}, {int(o1["T"][0])}  nan_state {int(o0["nan_state"][0])}, {int(o1["nan_state"][0])}',
              flush=True)
    rec.save(args.out, flat, STEM)


if __name__ == '__main__':
    main()
