"""Measure how much of the per-iteration bars the BAMP / SCAMP engines use (MI355X).
  python tools/launch_iter_err.py [OUT]      (default: profiles/launch_iter_err.txt)

One line per (algorithm, engine, case, arithmetic), iteration and quantity of
tests/test_gpu_bamp_iter.py, test_gpu_scamp_iter.py and test_gpu_scamp_persist_iter.py:
  xmap, psi      the engine's rms / worst-block rms / max error against the float64 step on its own
                 outputs, as multiples of the numpy c64 step's on the identical inputs (bars: K_RMS,
                 K_RMS, K_MAX of tests/persist_linear_ref.py), and the two rms themselves (psi at
                 t=0: a forward with fewer than 16 psi values per iteration, all iterations at once);
  xmmse, var     the largest deviation from the float64 denoiser as a fraction of its bar
                 (3e-6 + 4e-7 max|xi|, for var plus 1e-4 |ref|).
A summary per engine follows (the worst rms and max ratios).  Every assertion of the tests runs on
every forward measured here (the bars after the table is written)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, '..', 'tests'), os.path.join(HERE, '..'),
                os.path.join(HERE, '..', 'amp-sparc-spatialmodulation_amd')]
import torch  # noqa: E402
import launch_iter_gpu as lig  # noqa: E402
import launch_iter_ref as lir  # noqa: E402


def rows(who, lin, den):
    out = []
    for r in lin:
        out.append(f'{who:74s} t={r.t} {r.what:5s} | rms x{r.rms:5.2f}  block x{r.blk:5.2f}  max x{r.max:5.2f} | '
                   f'rms {r.got.rms:.2e}  numpy {r.yard.rms:.2e}')
    for r in den:
        v = '' if r.var is None else f'  var {r.var:.3f}'
        out.append(f'{who:74s} t={r.t} {r.what:9s} | of the bar: x {r.x:.3f}{v}  (max|xi| {r.max_abs_xi:.1f})')
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, '..', 'profiles', 'launch_iter_err.txt')
    device = torch.device('cuda:0')
    lines = ['# algorithm engine case arithmetic iteration quantity | ratio to the numpy c64 step: rms, worst 32 x 64 '
             'block rms, max | rms: engine, numpy',
             f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); seed {lir.SEED}, '
             f'{lir.T} iterations; bars: rms and block x{lir.K_RMS:g}, max x{lir.K_MAX:g}; denoiser fractions <= 1']
    jobs = [('bamp launches', lambda c=c, g=g: lig.measure_bamp(device, c, g))
            for c in lir.BAMP_CASES for g in lir.bamp_arithmetics(c)]
    jobs += [('scamp launches', lambda c=c, g=g: lig.measure_scamp(device, c, g, lir.ENGINE_LAUNCHES))
             for c in lir.SCAMP_CASES for g in lir.scamp_arithmetics(c)]
    jobs += [('scamp persistent', lambda c=c, g=g: lig.measure_scamp(device, c, g, lir.ENGINE_PERSISTENT))
             for c in lir.PERSIST_CASES for g in (lir.GEMM_F32, lir.GEMM_X3, lir.GEMM_H2)]
    done, worst, failed = [], {}, []
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for engine, job in jobs:
        try:
            who, lin, den = job()
        except AssertionError as e:      # a forward's status: reported, the table goes on
            failed.append(f'{engine}: {e}')
            lines.append(f'# FAILED {engine}: {e}')
            continue
        finally:
            with open(out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        done.append((who, lin, den))
        lines += rows(who, lin, den)
        w = worst.setdefault(engine, dict(rms=(0, ''), blk=(0, ''), max=(0, ''), x=(0, ''), var=(0, '')))
        for r in lin:
            for k in ('rms', 'blk', 'max'):
                w[k] = max(w[k], (getattr(r, k), f'{who} {r.what} t={r.t}'))
        for r in den:
            w['x'] = max(w['x'], (r.x, f'{who} t={r.t}'))
            if r.var is not None:
                w['var'] = max(w['var'], (r.var, f'{who} t={r.t}'))
    lines.append('# worst per engine')
    for engine, w in worst.items():
        lines.append(f'# {engine}: rms x{w["rms"][0]:.2f} ({w["rms"][1]}); block x{w["blk"][0]:.2f} ({w["blk"][1]}); '
                     f'max x{w["max"][0]:.2f} ({w["max"][1]}); denoiser x {w["x"][0]:.3f} ({w["x"][1]})'
                     + (f', var {w["var"][0]:.3f} ({w["var"][1]})' if w['var'][1] else ''))
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    assert not failed, failed
    for who, lin, den in done:       # the tests' bars, after the table is written
        lir.assert_bars(who, lin, den)


if __name__ == '__main__':
    main()
