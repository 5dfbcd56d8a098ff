"""Measure how much of the per-iteration bars the VAMP launch engine uses (MI355X).
  python tools/vamp_launch_iter_err.py [OUT]      (default: profiles/vamp_launch_iter_err.txt)

One line per case, phase and iteration of tests/test_gpu_vamp_launch_iter.py:
  y~, w, r       the engine's e_rms / worst 32 x 64 block rms / e_max against the float64 step on its
                 own state, as multiples of the numpy c64 step's on the identical inputs (bars: K_RMS,
                 K_RMS, K_MAX of tests/persist_linear_ref.py), and the two e_rms themselves;
  xmmse/var      the largest deviation from the float64 denoiser as a fraction of its bar
                 (3e-6 + 4e-7 max|xi|, for var plus 1e-4 |ref|).
The trial-sharded slices follow (r and the denoiser), then the worst ratios per phase.  Every
assertion of the test runs on every forward measured here (the bars after the table is written)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, '..', 'tests'), os.path.join(HERE, '..'),
                os.path.join(HERE, '..', 'amp-sparc-spatialmodulation_amd')]
import pytest  # noqa: E402
import torch  # noqa: E402
import vamp_launch_iter_gpu as vig  # noqa: E402
import vamp_launch_iter_ref as vir  # noqa: E402


def rows(who, lin, den):
    out = []
    for r in lin:
        out.append(f'{who:66s} t={r.t} {r.what:9s} | rms x{r.rms:5.2f}  block x{r.blk:5.2f}  max x{r.max:5.2f} | '
                   f'e_rms {r.got[1]:.2e}  numpy {r.yard[1]:.2e}')
    for r in den:
        out.append(f'{who:66s} t={r.t} {r.what:9s} | of the bar: x {r.x:.3f}  var {r.var:.3f}  (max|xi| {r.max_abs_xi:.1f})')
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, '..', 'profiles', 'vamp_launch_iter_err.txt')
    device = torch.device('cuda:0')
    lines = ['# case iteration phase | ratio to the numpy c64 step: e_rms, worst 32 x 64 block rms, e_max | e_rms: engine, numpy',
             f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); seed {vir.SEED}, '
             f'{vir.ITERS} iterations; bars: rms and block x{vir.K_RMS:g}, max x{vir.K_MAX:g}; denoiser fractions <= 1']
    jobs = [lambda c=c: [vig.measure(device, c)] for c in vir.CASES]
    mp = pytest.MonkeyPatch()
    jobs.append(lambda: vig.measure_sharded(device, mp))
    done, failed = [], []
    worst = {}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    try:
        for job in jobs:
            try:
                recs = job()
            except AssertionError as e:      # a forward's status or scalars: reported, the table goes on
                failed.append(str(e))
                lines.append(f'# FAILED: {e}')
                continue
            finally:
                with open(out, 'w') as f:
                    f.write('\n'.join(lines) + '\n')
            for who, lin, den in recs:
                done.append((who, lin, den))
                lines += rows(who, lin, den)
                for r in lin:
                    w = worst.setdefault(r.what, dict(rms=(0, ''), blk=(0, ''), max=(0, '')))
                    for k in ('rms', 'blk', 'max'):
                        w[k] = max(w[k], (getattr(r, k), f'{who} t={r.t}'))
                for r in den:
                    w = worst.setdefault('denoiser', dict(x=(0, ''), var=(0, '')))
                    w['x'] = max(w['x'], (r.x, f'{who} t={r.t}'))
                    w['var'] = max(w['var'], (r.var, f'{who} t={r.t}'))
    finally:
        mp.undo()
    lines.append('# worst per phase')
    for what, w in worst.items():
        if what == 'denoiser':
            lines.append(f'# denoiser: x {w["x"][0]:.3f} ({w["x"][1]}); var {w["var"][0]:.3f} ({w["var"][1]})')
        else:
            lines.append(f'# {what}: rms x{w["rms"][0]:.2f} ({w["rms"][1]}); block x{w["blk"][0]:.2f} ({w["blk"][1]}); '
                         f'max x{w["max"][0]:.2f} ({w["max"][1]})')
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    assert not failed, failed
    for who, lin, den in done:       # the test's bars, after the table is written
        vir.assert_bars(who, lin, den)


if __name__ == '__main__':
    main()
