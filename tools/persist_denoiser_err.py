"""Measure how much of the denoiser bars each persistent-engine form uses (MI355X).
  python tools/persist_denoiser_err.py [OUT]      (default: profiles/persist_denoiser_err.txt)

One line per (kernel class, alphabet, M) of tests/persist_denoiser_cases.py: the amp_denoise.h
form, max |xmmse - ref| / tolerance and max var error / its bar against the float64 denoiser on the
kernel's own input (the bars of tests/test_gpu_persist_denoiser.py assertion 1; over the three
iterations of a bf16x3 class, over the 1- and 3-iteration forwards of an f32 class), and the same
two ratios for amp_block_denoise (the U = 1 form of the g2 goldens) on the same r and tau as the
last iteration.  Reported, not asserted: the margin a later tightening can start from.  The
assertions of the test run on every forward measured here."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, '..', 'tests'), os.path.join(HERE, '..'),
                os.path.join(HERE, '..', 'amp-sparc-spatialmodulation_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import persist_denoiser_cases as pdc  # noqa: E402
import test_gpu_persist_denoiser as tpd  # noqa: E402
from vamp import block_denoise  # noqa: E402


def standalone(device, cfg, r2n, tau, M):
    """amp_block_denoise (mode 0) on r ([B, 2N] float32) at tau: its two error ratios."""
    r = tpd._cplx(r2n)
    rd = torch.from_numpy(r.astype(np.complex64)).to(device)
    xm, var = block_denoise(cfg, rd, float(tau), mode=0)
    ref = pdc.denoise_f64(r, np.float64(np.float32(tau)), cfg.symbols, cfg.Nt // M, M)
    return tpd.errors(xm.cpu().numpy()[..., 0].astype(np.complex128), var.cpu().numpy()[..., 0].astype(np.float64), ref)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, '..', 'profiles', 'persist_denoiser_err.txt')
    device = torch.device('cuda:0')
    lines = ['# class alphabet M form policy partial_round | persistent: x_err/tol var_err/bar | '
             'amp_block_denoise on the same r, tau: x_err/tol var_err/bar',
             f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); B = {pdc.B}, seed {pdc.SEED}, EbN0 {pdc.EBN0} dB, '
             f'{pdc.ITERS} iterations; tol = 3e-6 + 4e-7 max|xi|, var bar = 1e-4 |ref| + tol']
    for alphabet in pdc.ALPHABETS:
        for cls in pdc.CLASSES:
            for M in pdc.section_sizes(cls, alphabet):
                if pdc.CLASSES[cls][0] == pdc.GEMM_X3:
                    cap = tpd.capture_x3(device, cls, alphabet, M)
                    ratios = tpd.check_x3(cap, M)
                    last = pdc.ITERS - 1
                    sx, sv = standalone(device, cap.cfg, cap.r[last], np.float32(1.0) / np.float32(cap.inv[last]), M)
                else:
                    ratios = []
                    for iters in (1, pdc.ITERS):
                        cap = tpd.capture_f32(device, cls, alphabet, M, iters)
                        ratios.append(tpd.check_f32(cap, M, iters))
                    sx, sv = standalone(device, cap.cfg, cap.r, cap.status.last_scalar[2], M)
                ex, ev = max(a for a, _ in ratios), max(b for _, b in ratios)
                lines.append(f'{cls:9s} {alphabet:6s} M={M:<3d} {pdc.expected_form(cls, alphabet):18s} '
                             f'{pdc.packing(cls, alphabet):8s} {"partial" if pdc.partial_round(cls, alphabet, M) else "full   "}'
                             f' | {ex:6.3f} {ev:6.3f} | {sx:6.3f} {sv:6.3f}')
                print(lines[-1], flush=True)
    for alphabet, M in tpd.ST_CASES:
        res = tpd.standalone_errors(device, alphabet, M)
        form = 'M>64 per-point' if M > 64 else ('wide/grid/R8' if alphabet == 'sq64' else
                                                f'grid/R{pdc.grid_of(alphabet)[0]}/FULL/U1')
        lines.append(f'standalone {alphabet:6s} M={M:<3d} {form:18s} | ' +
                     ' | '.join(f'mode {m}: {a:6.3f} {b:6.3f}' for m, (a, b) in sorted(res.items())))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
