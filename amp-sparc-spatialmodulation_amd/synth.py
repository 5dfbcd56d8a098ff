"""Inputs of the trial batches drawn on the device (throughput mode): the input stage with the
granularity of ``forward_trials`` — all G channels of a call in one launch (amp_synth_channels)
and all E trials' x / sym / idx / noise / y in one launch (amp_synth_trials), in place of one
``Channel.generate_as_sparc`` per channel and one ``Data.generate_message`` + ``Channel.awgn`` +
dense ``A x`` per trial.

Same distributions as the reference's generators (channel.py:75-95, data.py:74-91 or, for
generator_mode 'random', data.py:55-72: an exactly uniform Na-subset of the Nt antennas per channel
use and one symbol for all of them, amp_synth_args.message = 1; channel.py:103-116), its own random stream: Philox4x32-10, every draw a pure function of
(seed, stream, id, index) (include/amp_sparc.h), so a trial's inputs do not depend on how the
trials are grouped into calls.  tests/synth_ref.py restates the mapping in numpy
(tests/synth_random_ref.py the 'random' message).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import amp_native as nat
from channel import Channel
from config import Config


class TrialSynth:
    def __init__(self, config: Config, seed: int) -> None:
        if not config.is_complex:
            raise ValueError('TrialSynth: the trial engines take complex64 inputs (is_complex=True)')
        self.config = config
        self.seed = int(seed) % 2 ** 64
        self.device = torch.device(config.device)
        W = Channel(config)._base_matrix()                      # channel.py:80-83
        self._W64 = W
        self._sw = None
        self._Wt = None

    def _base(self):
        """(W f32 [Lout, Lin], sqrt(W) f32) on the device, formed once."""
        if self._sw is None:
            self._Wt = torch.tensor(self._W64, dtype=torch.float32, device=self.device)
            self._sw = torch.tensor(np.sqrt(self._W64), dtype=torch.float32, device=self.device).contiguous()
        return self._Wt, self._sw

    def channels(self, G: int, channel0: int):
        """(W f32 [Lout, Lin], A c64 [G, n, N], At c64 [G, N, n]): the channels with ids channel0 ..
        channel0 + G - 1, as generate_as_sparc builds them, and their plain transposes."""
        cfg = self.config
        G = int(G)
        if G < 1:
            raise ValueError(f'TrialSynth.channels: G = {G} (>= 1)')
        d = cfg.dims(batch=1)
        W, sw = self._base()
        with torch.cuda.device(self.device):
            A = torch.empty(G, d.n, d.N, dtype=torch.complex64, device=self.device)
            At = torch.empty(G, d.N, d.n, dtype=torch.complex64, device=self.device)
            a = nat.AmpSynthArgs()
            a.seed, a.channel0 = self.seed, int(channel0) % 2 ** 64
            a.sw, a.A, a.At = nat.dptr(sw, torch.float32, 'sw'), nat.dptr(A), nat.dptr(At)
            a.Lh = cfg.Lh
            nat.check(nat.lib().amp_synth_channels(C.byref(d), C.byref(a), G, nat.stream_ptr(self.device)),
                      'amp_synth_channels')
        return W, A, At

    def trials(self, At: torch.Tensor, E: int, per_channel: int, SNR: float, trial0: int, band: bool = True,
               want_noise: bool = False):
        """(x c64 [E, N], sym int64 [E, L], idx int64 [E, L], y c64 [E, n] [, noise c64 [E, n]]) of
        the trials with ids trial0 .. trial0 + E - 1, trial e on channel At[e // per_channel]
        ([G, N, n], or one [N, n]); stacks that forward_trials takes as they are.  band: At comes
        from channels() or generate_as_sparc (only the Lh column blocks under a row are summed);
        band=False sums every section, for any channel."""
        cfg = self.config
        E, R = int(E), int(per_channel)
        if E < 1 or R < 1:
            raise ValueError(f'TrialSynth.trials: E = {E}, per_channel = {R} (both >= 1)')
        d = cfg.dims(batch=1)
        G = -(-E // R)
        if At.dim() == 2:
            At = At.unsqueeze(0)
        if tuple(At.shape) != (G, d.N, d.n):
            raise ValueError(f'TrialSynth.trials: At has shape {tuple(At.shape)}, expected {(G, d.N, d.n)} '
                             f'(trial e uses channel e // per_channel: {G} channels for {E} trials)')
        dev = At.device
        with torch.cuda.device(dev):
            x = torch.empty(E, d.N, dtype=torch.complex64, device=dev)
            sym = torch.empty(E, d.L, dtype=torch.int64, device=dev)
            idx = torch.empty(E, d.L, dtype=torch.int64, device=dev)
            y = torch.empty(E, d.n, dtype=torch.complex64, device=dev)
            noise = torch.empty(E, d.n, dtype=torch.complex64, device=dev) if want_noise else None
            a = nat.AmpSynthArgs()
            a.seed, a.trial0 = self.seed, int(trial0) % 2 ** 64
            a.At = nat.dptr(At, torch.complex64, 'At')
            a.band_blocks = cfg.Lh if band else 0
            a.noise_std = float(np.sqrt(cfg.Na / cfg.Nr / SNR / 2))          # channel.py:153
            a.message = 1 if cfg.mode == 'random' else 0                     # Data.random / Data.segmented
            a.x, a.sym, a.idx, a.y = nat.dptr(x), nat.dptr(sym), nat.dptr(idx), nat.dptr(y)
            a.noise = nat.dptr(noise) if want_noise else None
            cst = cfg.constellation()
            nat.check(nat.lib().amp_synth_trials(C.byref(d), C.byref(cst), C.byref(a), E, R, nat.stream_ptr(dev)),
                      'amp_synth_trials')
        return (x, sym, idx, y, noise) if want_noise else (x, sym, idx, y)
