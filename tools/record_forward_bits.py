#!/usr/bin/env python3
"""Records the bits of a building and of a reuse VAMP forward, with their inputs, as the fixture of
tests/test_gpu_vamp_ring_prefill.py (tests/golden/ring_prefill_bits.part<k>.npz).

  python tools/record_forward_bits.py [--out DIR] [--stem STEM] [--cases "Nt,Na,Nr,B,alphabet;..."] [--share-channel]
                                      [--ebn0 "dB;..."] [--nan-row "row;..."] [--inf-entry "row,col;..."]
                                      [--scale-y "f;..."] [--dump] [--dump-wr]
                                      [--tail] [--iters "n;..."] [--tags "tag;..."] [--forwards n]

--stem / --cases record another fixture (tests/golden/<stem>.part<k>.npz) for another case list;
--share-channel draws one channel, the first case's, stores it once ('shared/U', 's', 'Vh', 'SNR')
and runs every case that agrees with it in Nt and Nr on it (another case draws and stores its own);
--ebn0 sets Eb/N0 per case (one value: every case; an empty entry: the alphabet's default) and
stores that case's SNR as '<case>/SNR', e.g. to record a forward that stops before the cap;
--nan-row sets one row of y to NaN per case (an empty entry: none), in both forwards;
--inf-entry sets one entry of y to +inf per case ("row,col"; an empty entry: none), in both forwards;
--scale-y multiplies y of a case by f (an empty entry: 1), in both forwards, with the noise variance left
at the channel's: the logits grow with f, which drives a case into the exact-float64 rare path;
--dump-wr runs both forwards with the state dump on and stores each forward's GEMM1 epilogue w and
GEMM2 epilogue r per iteration: the first WR_FULL iterations whole ('f<i>_it_w', 'f<i>_it_r'
[WR_FULL, B, 2N]), every iteration as one CRC-32 per trial row ('f<i>_it_wcrc', 'f<i>_it_rcrc' [T, B])
and whether the row of w is finite ('f<i>_it_wfin');
--tail runs every forward with the state dump on and stores, per iteration, one CRC-32 per trial row of the
GEMM1 epilogue's w ('f<i>_it_wcrc' [T, B]; w carries vr and the LMMSE reciprocal of its column), whether the
row is finite ('f<i>_it_wfin') and each workgroup's 1 / sigma2 as the denoiser took it ('f<i>_it_inv' [T, nwg]),
and the status record's four scalars ('f<i>_last_scalar');
--iters sets the iteration cap per case (one value: every case; an empty entry: 20);
--tags appends '#<tag>' to a case's name in the fixture, so that one shape can be recorded several times
(another cap, Eb/N0 or y); --forwards n records n forwards per case (the first builds, the others reuse);
--dump runs the reuse forward with the persistent engine's per-iteration state dump on and stores,
for the iterations it ran, every valid trial's var ('f1_it_var'), each wave's float64 var sum
('f1_it_wsum') and the exchange records the workgroups published ('f1_it_gran').

Public API only (Config, Channel, Data, VAMP, amp_native.prepare_counts), so the same script runs
on any commit: a change that must leave the engine's results bit-identical is checked against a
fixture recorded on its parent.  The inputs (U, s, Vh, y, x, sym, idx) are stored too: LAPACK's SVD
is not pinned across hosts.  Arrays larger than CHUNK bytes are stored in row blocks
('<case>/<field>@<i>'), and the parts are filled greedily up to PART_LIMIT bytes each.
"""
import argparse
import io
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'amp-sparc-spatialmodulation_amd'))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch        # noqa: E402

STEM = 'ring_prefill_bits'
PART_LIMIT = 1000000
CHUNK = 300000
# (Nt, Na, Nr, B, alphabet): G3 = Nt / 32 reduction groups per GEMM
CASES = [(64, 4, 128, 40, '16QAM'), (64, 4, 128, 40, 'QPSK'), (128, 4, 256, 16, '16QAM'), (256, 8, 512, 32, '16QAM')]
EBN0 = {'16QAM': 10.0, 'QPSK': 6.0}
SEED = 23


def case_name(Nt, Na, Nr, B, alphabet):
    return f'{alphabet}_{Nt}_{Na}_{Nr}_{B}'


def config(Nt, Na, Nr, B, alphabet, device, iterations=20):
    from config import Config
    return Config(Nt, Na, Nr, 1, 1, batch=B, generator_mode='sparc', iterations=iterations, alphabet=alphabet,
                  channel_profile='uniform', channel_truncation='tail', device=device)


def make_inputs(case, shared=None, ebn0=None, nan_row=None, inf_entry=None, scale_y=None, forwards=2):
    """One channel and two (forwards) epochs of messages + noise (host tensors), in the reference's call order.
    shared: the make_inputs result of another case whose channel (A, U, s, Vh, SNR) this one uses;
    ebn0: this case's own Eb/N0 (else the alphabet's default, or the shared channel's SNR);
    nan_row: the row of y set to NaN in both epochs; inf_entry: the (row, column) of y set to +inf in both;
    scale_y: the factor y is multiplied by in both (before nan_row / inf_entry)."""
    from channel import Channel
    from data import Data
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    c = config(*case, device='cpu')
    ch, da = Channel(c), Data(c)
    if shared is None:
        _, A = ch.generate_as_sparc()
        U, s, Vh = torch.linalg.svd(A, full_matrices=False)
        SNR = c.snr(EBN0[case[4]] if ebn0 is None else ebn0)
    else:
        A, U, s, Vh, SNR = (shared[k] for k in ('A', 'U', 's', 'Vh', 'SNR'))
    if ebn0 is not None:
        SNR = c.snr(ebn0)
    eps = []
    for _ in range(forwards):
        x, sym, idx = da.generate_message()
        y = A @ x + ch.awgn(SNR)
        if scale_y is not None:
            y = y * scale_y
        if nan_row is not None:
            y[nan_row] = float('nan')
        if inf_entry is not None:
            y[inf_entry[0], inf_entry[1]] = float('inf')
        eps.append(dict(x=x, sym=sym, idx=idx, y=y))
    return dict(A=A, U=U, s=s, Vh=Vh, SNR=SNR, eps=eps)


def forward(det, chan, SNR, ep, device):
    """One forward: (building prepares, reuse prepares) it made and its result arrays."""
    import amp_native as nat
    from loss import counts_to_vector
    b0, r0 = nat.prepare_counts()
    L = det(chan[0], chan[1], chan[2], ep['y'].to(device).contiguous(), SNR, ep['x'].to(device).contiguous(),
            ep['sym'], ep['idx'])
    L.resolve()
    b1, r1 = nat.prepare_counts()
    out = dict(r=torch.view_as_real(det.last.r.squeeze(-1).contiguous()).cpu().numpy().copy(),
               xmmse=torch.view_as_real(det.last.xmmse.squeeze(-1).contiguous()).cpu().numpy().copy(),
               var=det.last.var.squeeze(-1).cpu().numpy().copy(),
               T=np.array([int(L.last_status.T)]), nan_state=np.array([int(L.last_status.nan_state)]), counts=np.asarray(counts_to_vector(L.last_counts)))
    return (b1 - b0, r1 - r0), out


PBM = 16     # trials per persistent workgroup (csrc/amp_vamp.h)
ITERS = 20   # config()'s iteration cap


WR_FULL = 2  # iterations whose w and r --dump-wr stores whole


def row_crc(a):
    """CRC-32 of each row's bytes: a [T, B, n] -> uint32 [T, B]."""
    import zlib
    a = np.ascontiguousarray(a)
    return np.array([[zlib.crc32(r.tobytes()) for r in it] for it in a], dtype=np.uint32).reshape(a.shape[:2])


def dumped_forward(det, cfg, chan, SNR, ep, device, wr=False, tail=False):
    """forward() with the persistent engine's state dump on (amp_vamp_debug_dump); adds, for the
    iterations that ran: it_var [T, B, N] float32, it_wsum [T, nwg, waves] float64 (each wave's var
    sum), it_gran [T, nwg, 8] uint32 (the exchange records: sumvar, notclose, tag, max|xi|, min max, 0, tag)."""
    import ctypes as C
    import amp_native as nat
    B, N = cfg.B, cfg.dims().N
    nwg = -(-B // PBM)
    dump = torch.zeros(ITERS, nwg, 5, PBM, 2 * N, dtype=torch.float32, device=device)
    nat.check(nat.lib().amp_vamp_debug_dump(C.c_void_p(dump.data_ptr())), 'amp_vamp_debug_dump')
    try:
        made, out = forward(det, chan, SNR, ep, device)
        torch.cuda.synchronize()
    finally:
        nat.lib().amp_vamp_debug_dump(None)
    T = int(out['T'][0])
    assert int(det.last.status().gemm) == 2, 'the dump is the persistent bf16x3 engine\'s'
    d = dump.cpu().numpy()
    rows = [min(PBM, B - w * PBM) for w in range(nwg)]
    if tail:   # slot 0: w; slot 3, row 1, column N: the 1 / sigma2 the denoiser of this workgroup took
        w = np.concatenate([d[:T, g, 0, :rows[g]] for g in range(nwg)], axis=1)
        out['it_wcrc'], out['it_wfin'] = row_crc(w), np.isfinite(w).all(axis=2)
        out['it_inv'] = d[:T, :, 3, 1, N].copy()
        out['last_scalar'] = np.array(list(det.last.status().last_scalar), dtype=np.float32)
        return made, out
    off = (C.c_uint64 * 5)()
    nat.check(nat.lib().amp_vamp_debug_offsets(C.byref(cfg.dims()), N, ITERS, 1, off), 'amp_vamp_debug_offsets')
    gran = det.last.buf.ws[int(off[0]):int(off[0]) + ITERS * nwg * 32].cpu().numpy().view(np.uint32).reshape(ITERS, nwg, 8)
    waves = 8 if N >= 256 else 4
    out['it_var'] = np.concatenate([d[:T, w, 3, :rows[w], :N] for w in range(nwg)], axis=1).copy()
    out['it_wsum'] = np.ascontiguousarray(d[:T, :, 3, 0, N:N + 2 * waves]).view(np.float64).copy()
    out['it_gran'] = gran[:T].copy()
    if wr:   # slot 0: w (GEMM1's epilogue), slot 1: r (GEMM2's), both [16, 2N] per workgroup
        w, r = (np.concatenate([d[:T, g, slot, :rows[g]] for g in range(nwg)], axis=1) for slot in (0, 1))
        out['it_w'], out['it_r'] = w[:WR_FULL].copy(), r[:WR_FULL].copy()
        out['it_wcrc'], out['it_rcrc'] = row_crc(w), row_crc(r)
        out['it_wfin'] = np.isfinite(w).all(axis=2)
    return made, out


def run_case(case, inp, device, dump=False, wr=False, tail=False, iters=ITERS):
    """A building forward, then a reuse forward with a new y on the same channel objects
    (dump: the reuse forward with the state dump on; wr: both, with w and r stored too;
    tail: every forward of inp, dumped as --tail says; iters: the iteration cap, at most ITERS)."""
    from vamp import VAMP
    cfg = config(*case, device='cuda', iterations=iters)
    det = VAMP(cfg)
    chan = tuple(inp[k].to(device).contiguous() for k in ('U', 's', 'Vh'))
    if tail:
        return [dumped_forward(det, cfg, chan, inp['SNR'], ep, device, tail=True) for ep in inp['eps']]
    if wr:
        return [dumped_forward(det, cfg, chan, inp['SNR'], ep, device, wr=True) for ep in inp['eps']]
    res = [forward(det, chan, inp['SNR'], inp['eps'][0], device)]
    if dump:
        res.append(dumped_forward(det, cfg, chan, inp['SNR'], inp['eps'][1], device))
    else:
        res.append(forward(det, chan, inp['SNR'], inp['eps'][1], device))
    return res


def as_np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def chunked(name, a):
    a = np.ascontiguousarray(a)
    if a.nbytes <= CHUNK or a.ndim == 0 or a.shape[0] < 2:
        return {name: a}
    n = min(a.shape[0], -(-a.nbytes // CHUNK))
    return {f'{name}@{i}': b for i, b in enumerate(np.array_split(a, n, axis=0))}


def packed(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def save(out, flat, stem=STEM):
    parts, cur = [], {}
    for name, a in flat.items():
        for k, b in chunked(name, a).items():
            if cur and len(packed({**cur, k: b})) > PART_LIMIT:
                parts.append(cur)
                cur = {}
            cur[k] = b
    parts.append(cur)
    os.makedirs(out, exist_ok=True)
    for k, arrays in enumerate(parts):
        raw = packed(arrays)
        assert len(raw) <= PART_LIMIT, (k, len(raw))
        with open(os.path.join(out, f'{stem}.part{k}.npz'), 'wb') as f:
            f.write(raw)
        print(f'{stem}.part{k}.npz: {len(raw)} bytes, {len(arrays)} arrays')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    ap.add_argument('--stem', default=STEM)
    ap.add_argument('--cases', default=None, help='"Nt,Na,Nr,B,alphabet;..." (default: CASES)')
    ap.add_argument('--share-channel', action='store_true',
                    help="one channel, the first case's, stored once and used by every case")
    ap.add_argument('--ebn0', default=None, help='"dB;..." per case (one value: every case; empty: the default)')
    ap.add_argument('--nan-row', default=None, help='"row;..." per case: that row of y is NaN (empty: none)')
    ap.add_argument('--inf-entry', default=None, help='"row,col;..." per case: that entry of y is +inf (empty: none)')
    ap.add_argument('--scale-y', default=None, help='"f;..." per case: y is multiplied by f (empty: 1)')
    ap.add_argument('--dump-wr', action='store_true', help="both forwards' per-iteration w and r (see above)")
    ap.add_argument('--tail', action='store_true', help="every forward's per-iteration w CRCs and 1 / sigma2 (see above)")
    ap.add_argument('--iters', default=None, help='"n;..." per case: the iteration cap (one value: every case; empty: 20)')
    ap.add_argument('--tags', default=None, help='"tag;..." per case: the name\'s suffix in the fixture (empty: none)')
    ap.add_argument('--forwards', type=int, default=2, help='forwards per case (the first builds)')
    ap.add_argument('--dump', action='store_true', help="the reuse forward's per-iteration var, wave sums and exchange records")
    args = ap.parse_args()
    cases = CASES if args.cases is None else [
        tuple(int(v) for v in c.split(',')[:4]) + (c.split(',')[4],) for c in args.cases.split(';')]
    ebn0 = [None] * len(cases)
    if args.ebn0 is not None:
        vals = args.ebn0.split(';')
        vals = vals * len(cases) if len(vals) == 1 else vals
        assert len(vals) == len(cases), (vals, cases)
        ebn0 = [float(v) if v.strip() else None for v in vals]
    nan_rows = [None] * len(cases)
    if args.nan_row is not None:
        vals = args.nan_row.split(';')
        assert len(vals) == len(cases), (vals, cases)
        nan_rows = [int(v) if v.strip() else None for v in vals]
    inf_entries = [None] * len(cases)
    if args.inf_entry is not None:
        vals = args.inf_entry.split(';')
        assert len(vals) == len(cases), (vals, cases)
        inf_entries = [tuple(int(u) for u in v.split(',')) if v.strip() else None for v in vals]
    scales = [None] * len(cases)
    if args.scale_y is not None:
        vals = args.scale_y.split(';')
        assert len(vals) == len(cases), (vals, cases)
        scales = [float(v) if v.strip() else None for v in vals]
    iters = [ITERS] * len(cases)
    if args.iters is not None:
        vals = args.iters.split(';')
        vals = vals * len(cases) if len(vals) == 1 else vals
        assert len(vals) == len(cases), (vals, cases)
        iters = [int(v) if v.strip() else ITERS for v in vals]
        assert all(1 <= v <= ITERS for v in iters), iters
    tags = [''] * len(cases)
    if args.tags is not None:
        tags = [v.strip() for v in args.tags.split(';')]
        assert len(tags) == len(cases), (tags, cases)
    device = torch.device('cuda', 0)
    flat = {}
    shared = None
    for case, eb, nr, ie, sc, it, tag in zip(cases, ebn0, nan_rows, inf_entries, scales, iters, tags):
        name = case_name(*case) + (f'#{tag}' if tag else '')
        assert f'{name}/f0_y' not in flat, f'{name}: recorded twice (--tags)'
        own = shared is not None and case[0:3:2] != shared['dims']   # another Nt, Nr: its own channel
        inp = make_inputs(case, None if own else shared, eb, nr, ie, sc, args.forwards)
        res = run_case(case, inp, device, args.dump, args.dump_wr, args.tail, it)
        print(name, 'prepares (building, reuse) per forward:', [m for m, _ in res],
              'T:', [int(o['T'][0]) for _, o in res], 'nan_state:', [int(o['nan_state'][0]) for _, o in res])
        if args.share_channel and shared is None:
            shared = dict(inp, dims=case[0:3:2])
        chan = 'shared' if args.share_channel and not own else name
        if eb is not None:
            flat[f'{name}/SNR'] = np.array([inp['SNR']], dtype=np.float64)
        if f'{chan}/U' not in flat:
            for k in ('U', 's', 'Vh'):
                flat[f'{chan}/{k}'] = as_np(inp[k])
            flat[f'{chan}/SNR'] = np.array([inp['SNR']], dtype=np.float64)
        for i, (ep, (made, o)) in enumerate(zip(inp['eps'], res)):
            for k in ('x', 'sym', 'idx', 'y'):
                flat[f'{name}/f{i}_{k}'] = as_np(ep[k])
            flat[f'{name}/f{i}_made'] = np.array(made, dtype=np.int64)
            for k, v in o.items():
                flat[f'{name}/f{i}_{k}'] = v
    save(args.out, flat, args.stem)


if __name__ == '__main__':
    main()
