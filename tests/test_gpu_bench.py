"""GPU: bench.py as a command.  A plain run prints the headline line only (no runs of their own for
the roofline or the CPU baseline), `--steps` is the number of timed forwards, and
`--dump-outputs DIR` writes what the last timed forward returned: float32 / float64 arrays equal,
bit for bit, to the same forward run here on the same seeded inputs.  `--full` adds the blocks
that take runs of their own.  cfg2 (Nt=64, B=1024) keeps each run to a few seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


def _bench(*extra):
    cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--config', 'cfg2', '--steps', '3',
           '--warmup', '1', '--prewarm-ms', '0', *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_dumps_last_step(device, tmp_path):
    sys.path.insert(0, REPO)
    import bench
    from config import Config
    from loss import counts_to_vector
    from vamp import VAMP

    res = _bench('--dump-outputs', str(tmp_path / 'out'))
    for k in HEADLINE:
        assert k in res, k
    assert res['steps'] == 3 and res['detail']['epochs'] == 3          # --steps sets the timed steps
    assert res['unit'] == 'symbol-vectors/s' and res['higher_is_better'] is True
    assert res['ms_per_step'] > 0 and res['value'] == pytest.approx(1024 / (res['ms_per_step'] * 1e-3))
    for k in ('roofline', 'cpu_baseline'):
        assert k not in res, k
    assert 'kernel_ms' not in res['detail']

    got = {f[:-4]: np.load(tmp_path / 'out' / f) for f in sorted(os.listdir(tmp_path / 'out'))}
    assert sorted(got) == ['T', 'counts', 'loss', 'r', 'var', 'xmmse']
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    # the same forward here, on the inputs bench.py draws for these arguments
    Nt, Na, Nr, B, alph, iters = bench.CONFIGS['cfg2']
    cfg = Config(Nt, Na, Nr, 1, 1, batch=B, generator_mode='sparc', iterations=iters, alphabet=alph,
                 channel_profile='uniform', channel_truncation='tail', device='cuda')
    inp = bench.make_inputs(cfg, 0, 8.0, device)
    det = VAMP(cfg)
    L = det(inp['U'], inp['s'], inp['Vh'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
    L.resolve()
    pairs = lambda t: torch.view_as_real(t.squeeze(-1).contiguous()).cpu().numpy()  # noqa: E731
    assert got['r'].shape == (B, Nt, 2) and got['var'].shape == (B, Nt)
    assert np.array_equal(got['r'], pairs(det.last.r), equal_nan=True)
    assert np.array_equal(got['xmmse'], pairs(det.last.xmmse), equal_nan=True)
    assert np.array_equal(got['var'], det.last.var.squeeze(-1).cpu().numpy(), equal_nan=True)
    assert np.array_equal(got['counts'], counts_to_vector(L.last_counts))
    assert got['T'][0] == L.last_status.T == res['detail']['T']
    assert np.nanmax(np.abs(got['r'])) > 0


def test_bench_full_adds_own_runs():
    res = _bench('--full', '--cpu-sample', '64')
    for k in HEADLINE:
        assert k in res, k
    assert res['roofline']['achieved'] > 0 and res['roofline']['gemm'] == res['dtype']
    assert res['detail']['kernel_ms']['forward'] > 0
    assert res['cpu_baseline']['value'] > 0
