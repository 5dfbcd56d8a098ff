"""GPU: the eight-wave bf16x3 VAMP engine at one workgroup per CU with a wave-priority policy in the full
rounds of its denoiser (AMP_X3_DEN_PRIO, amp_denoise.h DenPrio: s_setprio by the half of the SIMD's wave
pair a wave belongs to, at the top of a round and, in two forms, between the exponentials and the section
sums) computes the bits it computed before.

Only the time at which instructions issue may change, so every forward must equal, bit for bit, what the
commit before the change computed on an MI355X: r, xmmse and var bits, T, all 13 counters and
status.last_scalar, and from the state dump (amp_vamp_debug_dump), per iteration, every trial row of w
(one CRC-32 per row; w of iteration t + 1 carries the denoiser's xmmse, var and sumvar of iteration t) and
every workgroup's 1 / sigma2 as its denoiser took it.  Against tests/golden/den_prio_bits.part*.npz and
tests/golden/den_prio_cases_bits.part*.npz, recorded on that commit, through its library, with

  python tools/record_forward_bits.py --stem den_prio_bits --share-channel --tail --forwards 3 \\
      --cases "256,8,512,35,16QAM" --iters 4
  python tools/record_forward_bits.py --stem den_prio_cases_bits --share-channel --tail --forwards 1 \\
      --cases "256,8,512,17,16QAM;256,16,512,35,16QAM;256,4,512,35,16QAM;256,8,512,35,16QAM;256,8,512,35,16QAM;256,8,512,35,16QAM;256,8,512,35,QPSK" \\
      --ebn0 "8;8;8;8;8;8;0" --iters "4;4;4;1;2;4;20" --tags ";;;cap1;cap2;nan;" --nan-row ";;;;;20;"

All at N = k = 256, n = 512 (the only geometry these kernels take):
  16QAM_256_8_512_35          M = 32, the position-pair step (DEN_FAST_PAIR).  Workgroups of 16, 16 and 3 rows:
                              in the last one nsec = 24, so waves 0-5 have one full round and waves 6-7 none:
                              on two SIMDs only one half enters the loop, and a wave that never raised its
                              priority must leave at 0 all the same.  Three forwards: the first builds, two reuse;
  16QAM_256_8_512_17          the last workgroup holds one row (nsec = 8): two waves with a round;
  16QAM_256_16_512_35         M = 16: the full-round step on grid2_core (DEN_FAST_FULL's loop);
  16QAM_256_4_512_35          M = 64: the same loop with one section per wave step;
  ...#cap1, #cap2             iteration caps 1 and 2: the priority is 0 again where the loop is left for the
                              epilogue, and where iteration 1's GEMMs set their own;
  ...#nan                     row 20 of y is NaN (a full workgroup: every full round of it carries NaNs);
  QPSK_256_8_512_35           0 dB, stops before the cap (asserted).  Its kernel has no full-round step and gets
                              no policy; the case shows that it computes what it did.

Run once through A/B libraries of the other forms as well (profiles/r17_den_prio_ab.txt): forms 1 and 2 pass;
form 3 fails the #nan case alone (NaNs of the NaN row with another payload: the empty asm that holds its mid-step
s_setprio in place changes the operand order of the sums behind it), so forms 3 and 4 are timing-only forms.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import record_forward_bits as rec  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MAIN = (256, 8, 512, 35, '16QAM')
QPSK = (256, 8, 512, 35, 'QPSK')
# (stem, forwards, case, tag, iteration cap)
CASES = [('den_prio_bits', 3, MAIN, '', 4),
         ('den_prio_cases_bits', 1, (256, 8, 512, 17, '16QAM'), '', 4),
         ('den_prio_cases_bits', 1, (256, 16, 512, 35, '16QAM'), '', 4),
         ('den_prio_cases_bits', 1, (256, 4, 512, 35, '16QAM'), '', 4),
         ('den_prio_cases_bits', 1, MAIN, 'cap1', 1),
         ('den_prio_cases_bits', 1, MAIN, 'cap2', 2),
         ('den_prio_cases_bits', 1, MAIN, 'nan', 4),
         ('den_prio_cases_bits', 1, QPSK, '', 20)]
FIELDS = ('r', 'xmmse', 'var', 'T', 'nan_state', 'counts', 'last_scalar', 'it_wcrc', 'it_wfin', 'it_inv')
MADE = ((1, 0), (0, 1), (0, 1))

_FIX = {}


def _name(case, tag):
    return rec.case_name(*case) + (f'#{tag}' if tag else '')


def _fixture(stem):
    """{case or 'shared': {field: array}} of a stem's parts, row blocks ('field@i') joined (read once)."""
    if stem not in _FIX:
        raw, k = {}, 0
        while os.path.exists(os.path.join(GOLDEN, f'{stem}.part{k}.npz')):
            z = np.load(os.path.join(GOLDEN, f'{stem}.part{k}.npz'))
            raw.update({n: z[n] for n in z.files})
            k += 1
        assert k, f'no fixture parts of {stem}'
        blocks, fix = {}, {}
        for n, a in raw.items():
            base, _, i = n.partition('@')
            blocks.setdefault(base, []).append((int(i or 0), a))
        for base, bl in blocks.items():
            case, field = base.split('/', 1)
            bl.sort(key=lambda p: p[0])
            fix.setdefault(case, {})[field] = bl[0][1] if len(bl) == 1 else np.concatenate([a for _, a in bl], axis=0)
        _FIX[stem] = fix
    return _FIX[stem]


def _diff(got, want, fields=FIELDS):
    """Every differing array and its first differing index (bitwise)."""
    bad = []
    for name in fields:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(f'{name}: {a.dtype}{a.shape} != {b.dtype}{b.shape}')
            continue
        ne = a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)
        if ne.any():
            i = int(np.flatnonzero(ne)[0]) // a.dtype.itemsize
            where = f' = [iteration, row or workgroup] {np.unravel_index(i, a.shape)}' if name.startswith('it_') else ''
            bad.append(f'{name}: first difference at flat index {i} of {a.size}{where} '
                       f'({a.reshape(-1)[i]!r} != {b.reshape(-1)[i]!r})')
    return bad


def _inputs(fix, case, tag, forwards):
    fx = fix[_name(case, tag)]
    ch = fx if 'U' in fx else fix['shared']             # its own channel, or the shared one
    snr = fx['SNR'] if 'SNR' in fx else ch['SNR']       # its own Eb/N0, or the channel's
    return fx, dict(U=torch.from_numpy(ch['U']), s=torch.from_numpy(ch['s']), Vh=torch.from_numpy(ch['Vh']),
                    SNR=float(snr[0]),
                    eps=[dict(x=torch.from_numpy(fx[f'f{i}_x']), sym=fx[f'f{i}_sym'], idx=fx[f'f{i}_idx'],
                              y=torch.from_numpy(fx[f'f{i}_y'])) for i in range(forwards)])


def test_the_fixtures_hold_the_cases_they_are_for():
    T = {}
    for stem, forwards, case, tag, cap in CASES:
        fx = _fixture(stem)[_name(case, tag)]
        nwg = -(-case[3] // rec.PBM)
        T[_name(case, tag)] = [int(fx[f'f{i}_T'][0]) for i in range(forwards)]
        for i in range(forwards):   # one record per (iteration, trial) and per (iteration, workgroup)
            t = T[_name(case, tag)][i]
            assert fx[f'f{i}_it_wcrc'].shape == (t, case[3]) and fx[f'f{i}_it_inv'].shape == (t, nwg)
            assert tuple(int(v) for v in fx[f'f{i}_made']) == MADE[i]
        if case[4] == '16QAM':
            assert T[_name(case, tag)] == [cap] * forwards, 'the 16-QAM forwards run to their cap'
    print(T)
    assert 1 < T[_name(QPSK, '')][0] < 20, 'the QPSK forward stops before the cap'
    bad = _fixture('den_prio_cases_bits')[_name(MAIN, 'nan')]
    y = bad['f0_y'].reshape(MAIN[3], -1)
    assert np.isnan(y[20]).all() and np.isfinite(np.delete(y, 20, axis=0)).all()
    assert not bad['f0_it_wfin'].all() and int(bad['f0_nan_state'][0]) != 0


@pytest.mark.parametrize('stem,forwards,case,tag,iters', CASES, ids=[_name(c, tag) for _, _, c, tag, _ in CASES])
def test_forward_and_dump_bits_equal_the_parent_commits(device, stem, forwards, case, tag, iters):
    fx, inp = _inputs(_fixture(stem), case, tag, forwards)
    res = rec.run_case(case, inp, device, tail=True, iters=iters)
    assert len(res) == forwards
    bad = []
    for i, (made, got) in enumerate(res):
        assert made == MADE[i], (i, made)
        want = {k: fx[f'f{i}_{k}'] for k in FIELDS}
        print(f'forward {i}: T {int(got["T"][0])} (fixture {int(want["T"][0])}) nan_state {int(got["nan_state"][0])} '
              f'(fixture {int(want["nan_state"][0])})')
        bad += [f'forward {i} ({"building" if i == 0 else "reuse"}): {m}' for m in _diff(got, want)]
    assert not bad, '\n'.join(bad)
