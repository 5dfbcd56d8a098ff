"""GPU: the BAMP, SCAMP and VAMP launch engines and their independent-trial engines compute the bits
they computed before their GEMM epilogues were shared (one __device__ body per epilogue, called by
the batch kernel and by the trial kernel with a compile-time row guard).

test_gpu_trials.py, test_gpu_bamp_wide.py and test_gpu_scamp_trials.py compare a trial with its own
B = 1 forward on the SAME build: a change of the shared body that moved both would pass them.  Here
every case is compared with tests/golden/launch_engine_bits.part*.npz, recorded on the commit before
the change, on an MI355X, with

  python tools/record_launch_engine_bits.py

T, nan_state, the 13 counters, xmap, xmmse and var (BAMP) / psi (SCAMP) must be bit-equal
(golden_io.bits_equal), and the arithmetic the Loss reports the same.  The cases (record_launch_engine_bits.CASES;
dims are Config(Nt, Na, Nr, Lin, Lh); batch cases B = 40: two row tiles, the second partial; trials cases E = 40;
20 iterations):
  BAMP f32, odd n, a partial last column tile, banded    (6,3,5,3,1) OOK, (48,6,12,2,2) OOK,
                                                          (12,3,5,2,2) QPSK (N % 4 == 2: the pair loader)
  BAMP wide tile (bn = 256, M = 128), dense               (256,2,32,1,1) QPSK
  BAMP split-precision forms, batch only                  (64,4,64,1,1) 16-QAM, gemm x3 and h2
  BAMP element-wise denoiser ('random', B = 1)            (48,6,12,2,2) QPSK
  SCAMP, psi formed in the tile                           (16,4,6,2,2) BPSK, (32,4,8,2,2) QPSK
  SCAMP, psi split                                        (192,12,24,3,2) QPSK, (96,6,12,4,2) OOK
  SCAMP wide tile                                         (256,2,32,1,1) QPSK
  SCAMP launch engine, gemm x3, batch only                (64,4,64,1,1) 16-QAM at 10 dB (the detector diverges there:
                                                          every entry NaN) and at 16 dB
  the float64 fix-up, BAMP and SCAMP                      (16,4,6,2,2) BPSK, 2 iterations, row 5's y scaled by
                                                          the stored factor (the recorder asserts nan_state 1
                                                          and some, not all, entries NaN)
each as a batch and as trials unless said otherwise.

VAMP (record_launch_engine_bits.VAMP_CASES, tests/golden/vamp_launch_bits.part*.npz, recorded on the commit
before its launch-engine bodies moved into amp_vamp_launch.h, with --stem vamp_launch_bits): r, xmmse and var in
place of xmap, xmmse and the state; VAMP(cfg, engine=ENGINE_LAUNCHES, gemm=GEMM_F32) as a batch, the same
detector at B = 1 with forward_trials as trials, ShardedVAMP(cfg) in one process (identity hook: the only way to
vamp_xr1 .. xr4) as 'sharded':
  K = 1, odd n = k = 15, a partial last column tile        (6,3,5,3,1) OOK
  K = 4, odd k, trials exit at odd and at even T           (12,3,5,2,2) QPSK at 10 dB
  K = 2, n > N so k = N                                    (8,2,11,1,1) BPSK
  K = 8, M = 2, odd n = k = 27                             (24,12,9,2,2) 8PSK
  M = 128: the 256-column tile of K2                       (256,2,32,1,1) QPSK
  K = 16, a persistent-eligible shape, batch and trials    (64,4,64,1,1) 16-QAM
  the float64 fix-up (sharded: the rare path of xr2..xr4)  (16,2,7,4,2) OOK, 2 iterations, row 5's y scaled
  the all-NaN rule                                         (16,2,7,4,2) OOK, 2 iterations, row 5's y NaN (the recorder
                                                           asserts every entry of the batch, or of trial 5 alone, NaN)
K = 64 cannot be reached through Config (its alphabets stop at 16 points): the vamp_k2<*, 64> / tvamp_k2<*, 64>
instantiations are covered by the resource comparison in profiles/vamp_shared_epilogues_resources.txt only.
"""
import os
import sys

import numpy as np
import pytest
import torch

import golden_io as gio

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import record_launch_engine_bits as rec  # noqa: E402

_FIX = {}


def _fixture(stem=rec.STEM):
    """{case or input name: {field: array}} of the stem's parts, row blocks ('field@i') joined (read once)."""
    fix = _FIX.setdefault(stem, {})
    if not fix:
        parts = gio.Parts(stem)
        blocks = {}
        for n in parts.files:
            base, _, i = n.partition('@')
            blocks.setdefault(base, []).append((int(i or 0), parts[n]))
        for base, bl in blocks.items():
            group, field = base.split('/', 1)
            bl.sort(key=lambda p: p[0])
            fix.setdefault(group, {})[field] = bl[0][1] if len(bl) == 1 else np.concatenate([a for _, a in bl], axis=0)
    return fix


def _holds_every_case(cases, stem):
    fix = _fixture(stem)
    for c in cases:
        fx = fix[rec.case_name(c)]
        assert set(rec.out_fields(c) + ('arith',)) <= set(fx), (rec.case_name(c), sorted(fx))
        if c['fixup']:
            assert rec.reaches_fixup(c, fx) and float(fx['scale'][0]) >= 30.0, rec.case_name(c)
        if c['allnan']:
            assert rec.all_nan_rule(c, fx), rec.case_name(c)


def test_the_fixture_holds_every_case_and_its_fixups_reach_the_fixup():
    _holds_every_case(rec.CASES, rec.STEM)


def test_the_vamp_fixture_holds_every_case_and_its_fixups_reach_the_fixup():
    _holds_every_case(rec.VAMP_CASES, rec.VAMP_STEM)
    assert sum(c['fixup'] for c in rec.VAMP_CASES) == 3 and sum(c['allnan'] for c in rec.VAMP_CASES) == 3


def _bits_equal_the_fixture(device, c, stem):
    fix = _fixture(stem)
    fx = fix[rec.case_name(c)]
    got = rec.run_case(c, fix[rec.input_name(c)], device, float(fx['scale'][0]) if c['fixup'] else 1.0)
    arith = [str(np.asarray(v['arith']).reshape(-1)[0]) for v in (got, fx)]
    print(rec.case_name(c), 'T', got['T'].tolist(), 'fixture', fx['T'].tolist(), 'arith', arith)
    assert arith[0] == arith[1], arith
    bad = [k for k in rec.out_fields(c)
           if not gio.bits_equal(torch.from_numpy(np.ascontiguousarray(got[k])), torch.from_numpy(np.ascontiguousarray(fx[k])))]
    assert not bad, '\n'.join(rec.differing(got, fx))


@pytest.mark.parametrize('c', rec.CASES, ids=[rec.case_name(c) for c in rec.CASES])
def test_launch_engine_bits_equal_the_parent_commits(device, c):
    _bits_equal_the_fixture(device, c, rec.STEM)


@pytest.mark.parametrize('c', rec.VAMP_CASES, ids=[rec.case_name(c) for c in rec.VAMP_CASES])
def test_vamp_launch_engine_bits_equal_the_parent_commits(device, c):
    _bits_equal_the_fixture(device, c, rec.VAMP_STEM)
