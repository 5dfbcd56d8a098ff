"""Measure how much of the linear-half bars each persistent-engine arithmetic uses (MI355X).
  python tools/persist_linear_err.py [OUT]      (default: profiles/persist_linear_err.txt)

One line per (case, batch, arithmetic, forward) of tests/test_gpu_persist_linear.py and per phase
(y~, w, r; w+r for the f32 class): over the three iterations, the largest e_rms and e_max of the
engine as a multiple of the numpy c64 restatement's on the identical inputs (the test's bars are
K_RMS and K_MAX of tests/persist_linear_ref.py), and the engine's and numpy's largest e_rms
themselves (|z - z_float64| / max|z_float64| over the valid rows).  Every assertion of the test
runs on every forward measured here (the bars after the table is written)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, '..', 'tests'), os.path.join(HERE, '..'),
                os.path.join(HERE, '..', 'amp-sparc-spatialmodulation_amd')]
import torch  # noqa: E402
import persist_linear_ref as plr  # noqa: E402
import test_gpu_persist_linear as tpl  # noqa: E402


ALL = []


def rows(who, recs):
    out = []
    for phase in ('y~', 'w', 'r', 'w+r'):
        sel = [r for r in recs if r.phase == phase]
        if not sel:
            continue
        rms, mx = max(sel, key=lambda r: r.rms), max(sel, key=lambda r: r.max)
        out.append(f'{who:44s} {phase:4s} | e_rms x{rms.rms:5.2f} (t={rms.t})  e_max x{mx.max:5.2f} (t={mx.t}) | '
                   f'e_rms {max(r.got[1] for r in sel):.2e}  numpy {max(r.yard[1] for r in sel):.2e}')
        ALL.append((who, sel))
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, '..', 'profiles', 'persist_linear_err.txt')
    device = torch.device('cuda:0')
    lines = ['# case batch arithmetic [forward] phase | largest ratio to the numpy c64 restatement over the iterations '
             '| largest e_rms: engine, numpy',
             f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); seed {plr.SEED}, '
             f'EbN0 {plr.EBN0} dB, {plr.ITERS} iterations; bars: e_rms x{plr.K_RMS:g}, e_max x{plr.K_MAX:g}']
    for batch, cases in ((plr.B, plr.CASES), (1, plr.B1_CASES)):
        for case in cases:
            for arith in plr.ARITHMETICS:
                lines += rows(f'{plr.case_id(case)} B={batch} {arith}', tpl.measure(device, case, arith, batch))
    for case in tpl.REUSE:
        built, reused = tpl.measure_reuse(device, case)
        lines += rows(f'{plr.case_id(case)} B={plr.B} bf16x3 building', built)
        lines += rows(f'{plr.case_id(case)} B={plr.B} bf16x3 reuse', reused)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    for who, sel in ALL:       # the test's bars, after the table is written
        tpl._bar(sel, who)


if __name__ == '__main__':
    main()
