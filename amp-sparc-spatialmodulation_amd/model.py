"""Monte-Carlo driver — drop-in for the reference's ``Model`` (vamp_model.py:17-69,
bamp_model.py:16-68, scamp_model.py:16-67): the EbN0 sweep that calls the detector once
per epoch, accumulates its ``Loss``, averages, writes ``{EbN0dB}.json`` and stops early
once FER < 1e-3.

One process per GPU: with ``torch.distributed`` initialised, the epochs of an SNR point
are split over the ranks in blocks of ``res`` (one channel realisation per block, as
``i % res == 0`` regenerates it in the reference), every rank runs its blocks on its own
GPU with its own random stream, and one all-reduce of the accumulated metrics per SNR
point merges them before the average (the only exchange: Monte-Carlo epochs are
independent).  With one process the epoch loop and the random-call order are exactly the
reference's.
"""
from __future__ import annotations

import os

import numpy as np
import torch
from torch import nn

from channel import Channel
from config import Config
from data import Data
from loss import Loss

_DIRS = {'vamp': 'VAMP', 'bamp': 'BAMPfinal', 'scamp': 'SCAMP'}   # vamp_model.py:29 etc.


def _detector(name: str, config: Config, random_trials: bool = False):
    if name == 'vamp':
        from vamp import VAMP
        return VAMP(config)
    if name == 'bamp':
        from bamp import BAMP
        return BAMP(config, random_trials=True) if random_trials else BAMP(config)
    if name == 'scamp':
        from scamp import SCAMP
        return SCAMP(config)
    raise ValueError(f'unknown detector {name!r}')


def _dist():
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank(), torch.distributed.get_world_size()
    return 0, 1


def _comm_device():
    """Where a collective's tensor must live: the rank's GPU for RCCL ('nccl'), host for gloo."""
    if torch.distributed.get_backend() == 'nccl':
        return torch.device('cuda', torch.cuda.current_device())
    return torch.device('cpu')


def _broadcast_seed() -> int:
    """A fresh base seed drawn on rank 0 (OS entropy) and broadcast to every rank."""
    base = torch.tensor([int(np.random.SeedSequence().entropy % (2 ** 31))], dtype=torch.int64)
    base = base.to(_comm_device())
    torch.distributed.broadcast(base, src=0)
    return int(base.cpu().item())


_JACOBI_CHUNK_BYTES = 1 << 30     # svd_gram(method='jacobi'): the complex128 copies of one chunk of channels


def _jacobi_chunk(G: int, n: int, N: int) -> int:
    """Channels per solver call: the complex128 copies of a chunk (its Gram matrices, E, the solver's
    work matrix; one channel's A and other factor at a time) stay under 1 GiB, and the chunks of a
    stack are of equal size, so that no call is left with a handful of channels."""
    k = min(n, N)
    cap = max(1, (_JACOBI_CHUNK_BYTES - 32 * n * N) // (48 * k * k))
    return -(-G // -(-G // cap))


def _svd_jacobi(A: torch.Tensor, max_cond: float):
    """svd_gram(method='jacobi') on a [G, n, N] complex64 ROCm stack; None where the eigh path has
    to take over (k above the solver's cap)."""
    import ctypes as C
    import warnings
    import amp_native as nat
    G, n, N = A.shape
    k, tall = min(n, N), n >= N
    if k > nat.EIGH_MAX_K:
        return None
    lib = nat.lib()
    dev = A.device
    U = torch.empty(G, n, k, dtype=torch.complex64, device=dev)
    s = torch.empty(G, k, dtype=torch.float32, device=dev)
    Vh = torch.empty(G, k, N, dtype=torch.complex64, device=dev)
    info = torch.empty(G, 2, dtype=torch.int32, device=dev)
    s64 = torch.empty(G, k, dtype=torch.float64, device=dev)
    step = _jacobi_chunk(G, n, N)
    for g0 in range(0, G, step):
        g1 = min(G, g0 + step)
        gram = torch.empty(g1 - g0, k, k, dtype=torch.complex128, device=dev)
        # one 2-D product per channel: a channel's bits do not depend on how many share the call
        for g in range(g1 - g0):
            Ag = A[g0 + g].to(torch.complex128)
            torch.mm(Ag.mH, Ag, out=gram[g]) if tall else torch.mm(Ag, Ag.mH, out=gram[g])
        E = torch.empty_like(gram)
        w = s64[g0:g1]
        a = nat.AmpEighArgs()
        a.G, a.E = nat.dptr(gram, torch.complex128, 'gram'), nat.dptr(E, torch.complex128, 'E')
        a.w, a.info = nat.dptr(w, torch.float64, 'w'), nat.dptr(info[g0:g1], torch.int32, 'info')
        need = lib.amp_eigh_workspace_bytes(k, g1 - g0)
        ws = nat.WORKSPACE.get(dev, 'eigh', need)
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        a.tol, a.max_sweeps = 0.0, 0
        nat.check(lib.amp_eigh_run(C.byref(a), k, g1 - g0, nat.stream_ptr(dev)), 'amp_eigh_run')
        sg = w.sqrt()
        for g in range(g1 - g0):
            Ag = A[g0 + g].to(torch.complex128)
            if tall:                               # E = V:  U = A V / s
                U[g0 + g] = torch.mm(Ag, E[g]) / sg[g].unsqueeze(-2)
                Vh[g0 + g] = E[g].mH
            else:                                  # E = U:  Vh = U^H A / s
                U[g0 + g] = E[g]
                Vh[g0 + g] = torch.mm(E[g].mH, Ag) / sg[g].unsqueeze(-1)
        s[g0:g1] = sg
    # the existing max_cond rule, on the float64 singular values
    ok = s64[:, -1].sqrt() * max_cond > s64[:, 0].sqrt()
    bad = (info[:, 1] == 0) & ok
    state = torch.stack([ok.all(), bad.any()]).tolist()
    if not state[0]:
        return torch.linalg.svd(A, full_matrices=False)
    if state[1]:
        redo = torch.nonzero(bad).flatten().tolist()
        warnings.warn(f'svd_gram(method=\'jacobi\'): {len(redo)} of {G} channels did not converge; redone by the '
                      'eigh path', RuntimeWarning, stacklevel=3)
        for g in redo:
            U[g], s[g], Vh[g] = svd_gram(A[g], max_cond)
    return U, s, Vh


def svd_gram(A: torch.Tensor, max_cond: float = 20.0, method: str = 'eigh'):
    """Thin SVD of a full-rank matrix through the Hermitian eigendecomposition of its Gram matrix
    (the smaller of A^H A / A A^H; torch.linalg.eigh), for Model(rng='device'): on MI355X 6.8 ms
    per cfg4 channel (512 x 256 c64) against 28.9 ms for torch.linalg.svd, and closer to exact
    (max |U S Vh - A| / max |A| 1.5e-6 vs 4.8e-5, max |Vh Vh^H - I| 1.0e-6 vs 5.5e-5;
    tools/svd_bench.py).  Squaring the matrix squares its condition number (the
    factors' orthogonality error grows as eps kappa^2: 4e-6 at kappa 6), so a channel with
    s_max / s_min above `max_cond` falls back to torch.linalg.svd; a random SPARC channel with
    n = 2N (cfg2, cfg4) sits near kappa = 6, a square one near N.  Returns (U, s, Vh) as torch.linalg.svd(A,
    full_matrices=False): s descending, U [n, k], Vh [k, N], k = min(n, N).
    method='eigh' (default) is the path above.  method='jacobi' (a ROCm [n, N] or [G, n, N] complex64
    tensor; a CPU tensor raises ValueError: there is no CPU fallback) takes the eigendecomposition
    from the library's batched float64 Jacobi solver instead (amp_eigh_run, csrc/amp_eigh.hip), which
    works on the channels of a stack side by side where rocSOLVER's eigh runs them one after
    another: the smaller Gram matrix is formed in complex128 (one product per channel, in chunks of
    channels whose complex128 copies stay under 1 GiB), s = sqrt(w) in float64, and the other factor
    E^H A / s or A E / s is formed in COMPLEX128 as well, then everything is rounded to complex64 /
    float32: the factors come out at float32 rounding level.  The float64 Gram matrix
    keeps the small singular values the float32 one loses, so a larger max_cond may be passed with
    it (the solver itself gives up where s_min / s_max < 2^-20).  A channel that did not converge is
    redone by the eigh path, alone, with one RuntimeWarning per call; k above the solver's cap
    (AMP_EIGH_MAX_K = 640) uses the eigh path.  Channel g of a stack gets the bits of the 2-D call on
    A[g]."""
    if method not in ('eigh', 'jacobi'):
        raise ValueError(f"svd_gram: method must be 'eigh' or 'jacobi', got {method!r}")
    if method == 'jacobi':
        if A.device.type != 'cuda':
            raise ValueError(f"svd_gram(method='jacobi') needs a ROCm device tensor (got {A.device}); there is "
                             'no CPU fallback')
        if A.dtype != torch.complex64 or A.dim() not in (2, 3):
            raise ValueError(f"svd_gram(method='jacobi') takes a complex64 [n, N] or [G, n, N] tensor, got "
                             f'{A.dtype} {tuple(A.shape)}')
        out = _svd_jacobi(A if A.dim() == 3 else A.unsqueeze(0), max_cond)
        if out is not None:
            return out if A.dim() == 3 else tuple(f[0] for f in out)
    n, N = A.shape[-2], A.shape[-1]
    tall = n >= N
    G = A.mH @ A if tall else A @ A.mH
    w, E = torch.linalg.eigh(G)                    # ascending
    w, E = w.flip(-1), E.flip(-1)
    s = w.clamp_min(0).sqrt()
    if not bool((s[..., -1] * max_cond > s[..., 0]).all()):
        return torch.linalg.svd(A, full_matrices=False)
    sd = s.to(A.dtype)
    if tall:                                       # E = V:  U = A V / s
        return (A @ E) / sd.unsqueeze(-2), s, E.mH
    return E, s, (E.mH @ A) / sd.unsqueeze(-1)     # E = U:  Vh = U^H A / s


class Model(nn.Module):
    def __init__(self, config: Config, detector: str = 'vamp', path: str | None = None, amp=None,
                 seed: int | None = None, rng: str = 'host', group_epochs: bool = False,
                 shard: str = 'epochs', group_trials: int = 0, trial_channels: int = 0,
                 trials_ws_limit: int = 4 << 30, synth_trials: bool = False,
                 device_svd: str = 'eigh') -> None:
        """rng='host' (default): the reference's numpy / torch-CPU random streams, bit for bit
        (parity mode).  rng='device': channel, messages and noise drawn on the GPU and the SVD
        on the GPU through the Gram matrix's eigendecomposition (svd_gram; throughput mode: same
        distributions, different streams).
        group_epochs: VAMP detects up to max_epochs of its epochs side by side in one persistent
        launch (VAMP.forward_epochs: one channel per epoch, or one per `res` block; same results,
        fills the GPU at small B).
        group_trials (> 0, config.B == 1, VAMP / BAMP): the reference's own way to run — batch = 1,
        `res` epochs per channel (vamp_model.py:91, 98) — with the runs of epochs that share a
        channel detected as independent trials in one launch sequence (forward_trials), in chunks
        of at most group_trials; every trial keeps its own scalars, shift and exit, so the sweep
        equals the per-epoch loop.  res = 1 degenerates to single forward calls.  generator_mode
        'random' (BAMP only): the detector is built with random_trials=True and goes through the same
        grouping; parity mode keeps drawing Data.random in the reference's call order, throughput mode
        needs synth_trials (TrialSynth draws that message; Data has no device generator for it).
        trial_channels (> 0, with group_trials = n, VAMP / BAMP / SCAMP; opt-in): one forward_trials call
        may hold the trials of up to trial_channels whole `res` blocks, each with its own channel, and at
        most n trials (forward_trials(..., per_channel=res): amp_vamp_trials_ch_run /
        amp_bamp_trials_ch_run / amp_scamp_trials_ch_run), so the reference's default res = 1 is a
        channel per trial.  VAMP hands over each block's (U, s, Vh), its SVD taken per channel as in
        the per-epoch loop (vamp_model.py:45-61: channel, SVD, message, noise).  The
        inputs are still drawn in the reference's order and the Losses yielded in epoch order; a
        block longer than n goes through the single-channel chunks above.  The packed operators of G
        channels cost G times one channel's bytes: the channels per call are capped so that the
        library's workspace query stays under trials_ws_limit bytes (a setting; default 4 GiB: VAMP's
        three dense operators leave one channel per call at the published Nt = 1344 shape).
        A 'vamp' detector object without a true `trials_per_channel` attribute raises.
        synth_trials (opt-in; needs rng='device', group_trials > 0 and config.B == 1, else ValueError):
        the channels and the trials of every forward_trials call are drawn by TrialSynth (synth.py:
        one launch for the call's channels, one for its trials' x / sym / idx / noise / y) and handed
        over as stacks, VAMP's SVDs taken by svd_gram on the [G, n, N] stack.  Its stream is its own
        (Philox, seed = this rank's seed; trial id = (SNR-point index << 32) + epoch number, channel
        id = (point index << 32) + epoch // res), so the sweep's Losses do not depend on
        group_trials / trial_channels; every call, a single trial included, goes through
        forward_trials.  The channels' transposes count towards trials_ws_limit.
        device_svd (needs rng='device' and the VAMP detector, else ValueError): how svd_gram takes the
        channels' SVDs in throughput mode: 'eigh' (default: torch.linalg.eigh, the channels of a stack one
        after another) or 'jacobi' (opt-in: the library's batched float64 Jacobi solver, svd_gram(A,
        method='jacobi'): the channels of a stack side by side; factors at float32 rounding level, other
        phases and rounding than 'eigh', so the two settings' sweeps agree statistically, not bit for bit).
        Measured on an MI355X at the published 528 x 2560 shape (profiles/svd_jacobi_bench.jsonl, DESIGN.md
        §7), eigh / jacobi: 11.47 / 4.76 ms per channel with 10 channels per call, 11.43 / 3.21 with 84; VAMP
        end to end 11.65 / 3.24 ms per trial at res = 1 and 1.200 / 0.521 at res = 10.  It is SLOWER where a
        call holds a single channel: 11.95 / 25.65 ms for one channel alone (6.40 / 8.58 at cfg4's 512 x 256),
        0.170 / 0.295 ms per trial at res = 100 with group_trials = 100; so it is for synth_trials sweeps
        with several channels per call, not for the per-epoch loop.  TrialSynth's streams depend only on the seed, so a sweep
        with either setting sees the same inputs.
        shard (with torch.distributed): 'epochs' (default) gives each rank whole epochs with its
        own random stream and merges the metrics once per SNR point; 'trials' (SURVEY §8(e)
        exact-compat, VAMP / BAMP / SCAMP) gives every rank the SAME epochs (one seed) and splits each batch's
        trials over the ranks with the batch scalars all-reduced every iteration (ShardedVAMP),
        so the sweep equals the single-process sweep."""
        super().__init__()
        self.config = config
        self.detector = detector
        self.rate = config.code_rate
        self.shannon_limit = config.shannon_limit_dB
        self.min_snr = self.shannon_limit
        if shard not in ('epochs', 'trials'):
            raise ValueError(f"shard must be 'epochs' or 'trials', got {shard!r}")
        self.shard = shard
        if amp is None and shard == 'trials':
            if detector == 'vamp':
                from vamp import ShardedVAMP
                amp = ShardedVAMP(config)
            elif detector == 'bamp':
                from bamp import ShardedBAMP
                amp = ShardedBAMP(config)
            else:
                from scamp import ShardedSCAMP
                amp = ShardedSCAMP(config)
        # generator_mode 'random' is batched by BAMP(random_trials=True) alone (a detector passed in is used as given)
        rnd = bool(group_trials) and group_trials > 0 and detector == 'bamp' and config.mode == 'random' and config.B == 1
        self.amp = amp if amp is not None else _detector(detector, config, random_trials=rnd)
        self.loss = Loss(config)
        self.rng = rng
        if device_svd not in ('eigh', 'jacobi'):
            raise ValueError(f"device_svd must be 'eigh' or 'jacobi', got {device_svd!r}")
        if device_svd != 'eigh' and (rng != 'device' or detector != 'vamp'):
            raise ValueError("device_svd: the device-side SVD is taken for rng='device' and the VAMP detector only")
        self.device_svd = device_svd
        self.channel = Channel(config, rng=rng)
        self.data = Data(config, rng=rng)
        self.path = path if path is not None else f'Simulations/{_DIRS[detector]}/{config.name}'
        self.rank, self.world = _dist()
        # trial sharding: every rank draws the same epochs (rank-independent seeding), the
        # detector splits each batch; epoch sharding: one stream per rank
        self._stream_rank = 0 if shard == 'trials' else self.rank
        self._epoch_world = 1 if shard == 'trials' else self.world
        if seed is None and self.world > 1:
            # unseeded multi-rank sweep: every rank would start torch's and numpy's generators
            # from the same default state and draw the same epochs; rank 0 draws a base seed
            # and broadcasts it, so the ranks' streams are distinct
            seed = _broadcast_seed()
        self.seed = seed
        if seed is not None:
            # one independent stream per rank (rank 0 of a 1-process run = the plain seed)
            np.random.seed((seed + 7919 * self._stream_rank) % 2 ** 32)
            torch.manual_seed(seed + 7919 * self._stream_rank)
        if self.rank == 0:
            os.makedirs(self.path, exist_ok=True)
        self.group_cap = 0
        self._ch_ok = None
        if group_epochs:
            if detector != 'vamp' or not hasattr(self.amp, 'forward_epochs'):
                raise ValueError('group_epochs: side-by-side epochs are built for the VAMP detector')
            N, n = config.Nt * config.Lin, config.Nr * config.Lout
            self.group_cap = self.amp.max_epochs(min(n, N))
        self.trials_cap = 0
        self.channels_cap = 0
        self.trials_ws_limit = int(trials_ws_limit)
        self._blocks_cap = {}
        if trial_channels:
            if trial_channels < 0:
                raise ValueError(f'trial_channels must be >= 0, got {trial_channels}')
            if not group_trials:
                raise ValueError('trial_channels: set group_trials (the most trials per call) as well')
            if detector not in ('bamp', 'scamp') and not getattr(self.amp, 'trials_per_channel', False):
                raise ValueError('trial_channels: trial batches over several channels need a detector whose '
                                 'forward_trials takes per_channel (BAMP, SCAMP, and VAMP with trials_per_channel)')
            self.channels_cap = int(trial_channels)
        if group_trials:
            if group_trials < 0:
                raise ValueError(f'group_trials must be >= 0, got {group_trials}')
            dets = ('vamp', 'bamp', 'scamp') if self.channels_cap else ('vamp', 'bamp')
            if config.B != 1 or detector not in dets or not hasattr(self.amp, 'forward_trials'):
                raise ValueError('group_trials: independent-trial batches are built for the VAMP and BAMP '
                                 'detectors at config.B == 1 (SCAMP with trial_channels > 0)')
            if shard == 'trials' or group_epochs:
                raise ValueError('group_trials does not combine with group_epochs or trial sharding')
            self.trials_cap = int(group_trials)
        self.synth = None
        self._point = 0
        if synth_trials:
            if rng != 'device' or not self.trials_cap or config.B != 1:
                raise ValueError("synth_trials: the trial batches' inputs are drawn on the device for "
                                 "rng='device', group_trials > 0 and config.B == 1")
            from synth import TrialSynth
            if seed is None:
                seed = int(np.random.SeedSequence().entropy % 2 ** 63)
            self.synth = TrialSynth(config, seed + 7919 * self._stream_rank)

    # one epoch, in the reference's random-call order (vamp_model.py:55-61)
    def _epoch(self, SNR: float, new_channel: bool):
        x, sym, idx, y = self._inputs(SNR, new_channel)
        if self.detector == 'vamp':
            U, s, Vh = self._svd
            return self.amp(U, s, Vh, y, SNR, x, sym, idx)
        if self.detector == 'bamp':
            return self.amp(self._A, y, SNR, x, sym, idx)
        return self.amp(self._W, self._A, y, SNR, x, sym, idx)

    def _group(self, SNR: float, ids: list, res: int) -> list:
        """The epochs `ids` (this rank's, in order) detected side by side with VAMP's persistent
        launch (VAMP.forward_epochs): every epoch's inputs are drawn in the reference's call order
        (the channel first when i % res == 0, then message + noise), then the epochs are
        detected in chunks that fit one persistent grid — with one channel per epoch where the
        chunk spans several channels (the reference's default res = 1 redraws it every epoch).
        Results equal the sequential _epoch calls."""
        cap = max(1, self.group_cap)
        out = []
        for c0 in range(0, len(ids), cap):
            chunk = []
            for i in ids[c0:c0 + cap]:
                x, sym, idx, y = self._inputs(SNR, i % res == 0)
                chunk.append((x, sym, idx, y, self._svd))
            chans = [v[4] for v in chunk]
            if all(c is chans[0] for c in chans):
                runs = [chunk]
            elif self._per_epoch_channels():
                runs = [chunk]
            else:
                # this arithmetic / shape takes one shared channel per launch only (e.g. GEMM_F32, or
                # n != 2k): the chunk goes as runs of epochs that share a channel (single epochs at res = 1)
                runs, cur = [], [chunk[0]]
                for v in chunk[1:]:
                    if v[4] is cur[-1][4]:
                        cur.append(v)
                    else:
                        runs.append(cur)
                        cur = [v]
                runs.append(cur)
            for run in runs:
                cs = [v[4] for v in run]
                if all(c is cs[0] for c in cs):
                    U, s, Vh = cs[0]
                else:
                    U, s, Vh = [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs]
                out += self.amp.forward_epochs(U, s, Vh, [v[3] for v in run], SNR, [v[0] for v in run],
                                               [v[1] for v in run], [v[2] for v in run])
        return out

    def _group_trials(self, SNR: float, ids: list, res: int):
        """The epochs `ids` (this rank's, in order), each drawn in the reference's call order (the
        channel first when i % res == 0, then message + noise: vamp_model.py:55-61); the runs of
        epochs that share a channel go through forward_trials in chunks of at most trials_cap, a
        run of one through the plain forward.  Yields the epochs' Losses in order (the caller
        accumulates each before the next detection, as the per-epoch loop does)."""
        run = []

        def flush():
            if len(run) == 1:
                x, sym, idx, y = run[0]
                if self.detector == 'vamp':
                    yield self.amp(*self._svd, y, SNR, x, sym, idx)
                else:
                    yield self.amp(self._A, y, SNR, x, sym, idx)
            elif run:
                cols = [[v[j] for v in run] for j in (3, 0, 1, 2)]        # ys, xs, symbols, indices
                if self.detector == 'vamp':
                    yield from self.amp.forward_trials(*self._svd, cols[0], SNR, *cols[1:])
                else:
                    yield from self.amp.forward_trials(self._A, cols[0], SNR, *cols[1:])
            run.clear()

        for i in ids:
            new = i % res == 0
            if new or len(run) >= self.trials_cap:
                yield from flush()         # before the next channel replaces this run's
            run.append(self._inputs(SNR, new))
        yield from flush()

    def _blocks_per_call(self, res: int) -> int:
        """The most whole `res` blocks one forward_trials call holds: at most channels_cap blocks and
        trials_cap trials, and the workspace query of that call within trials_ws_limit (a detector
        without the query, such as a test's stand-in, is not capped by it)."""
        k = self._blocks_cap.get(res)
        if k is None:
            k = max(1, min(self.channels_cap, self.trials_cap // res))
            query = getattr(self.amp, 'trials_workspace_bytes', None)
            # synth_trials: each channel's transpose At [N, n] c64 is held beside the operators
            at = 8 * self.config.Nt * self.config.Lin * self.config.Nr * self.config.Lout if self.synth else 0
            while k > 1 and query is not None and query(k * res, res) + k * at > self.trials_ws_limit:
                k -= 1
            self._blocks_cap[res] = k
        return k

    def _detect_trials(self, SNR: float, chans: list, run: list, per_channel):
        """One detection of the trials `run` ([(x, sym, idx, y)]) on the channels `chans` (VAMP: each
        an (U, s, Vh)): the plain forward for one trial, the single-channel forward_trials for one
        channel, else the several-channel form."""
        head = (self._W,) if self.detector == 'scamp' else ()
        if len(run) == 1:
            x, sym, idx, y = run[0]
            ch = chans[0] if self.detector == 'vamp' else head + (chans[0],)
            yield self.amp(*ch, y, SNR, x, sym, idx)
            return
        cols = [[v[j] for v in run] for j in (3, 0, 1, 2)]        # ys, xs, symbols, indices
        if len(chans) == 1:
            ch = chans[0] if self.detector == 'vamp' else head + (chans[0],)
            yield from self.amp.forward_trials(*ch, cols[0], SNR, *cols[1:])
        elif self.detector == 'vamp':
            Us, ss, Vhs = ([c[j] for c in chans] for j in range(3))
            yield from self.amp.forward_trials(Us, ss, Vhs, cols[0], SNR, *cols[1:], per_channel=per_channel)
        else:
            yield from self.amp.forward_trials(*head, list(chans), cols[0], SNR, *cols[1:], per_channel=per_channel)

    def _group_trial_channels(self, SNR: float, ids: list, res: int):
        """_group_trials with several channels per call (trial_channels > 0): the epochs `ids`, each
        drawn in the reference's call order; up to _blocks_per_call(res) whole `res` blocks, each with
        its own channel, go through one forward_trials call (a short last block closes its call: trial
        e uses channel e // res).  A block longer than trials_cap goes through single-channel chunks.
        Yields the epochs' Losses in order."""
        chans, run = [], []

        def flush():
            if run:
                yield from self._detect_trials(SNR, chans, run, res)
            chans.clear()
            run.clear()

        if res > self.trials_cap:
            for i in ids:
                new = i % res == 0
                if new or len(run) >= self.trials_cap:
                    yield from flush()
                run.append(self._inputs(SNR, new))
                if not chans:
                    chans.append(self._svd if self.detector == 'vamp' else self._A)
            yield from flush()
            return
        cap = self._blocks_per_call(res)
        for i in ids:
            new = i % res == 0
            if new and len(chans) >= cap:
                yield from flush()
            run.append(self._inputs(SNR, new))
            if new or not chans:
                chans.append(self._svd if self.detector == 'vamp' else self._A)
        yield from flush()

    def _synth_calls(self, ids: list, res: int) -> list:
        """The forward_trials calls of the epochs `ids` under synth_trials: [(first epoch, trials,
        first block, blocks)].  Without trial_channels (or with a block longer than trials_cap) a
        call is a chunk of at most trials_cap epochs of one block; else up to _blocks_per_call(res)
        whole blocks whose epochs and block numbers run on consecutively (TrialSynth's ids are
        id0 + e and id0 + g), a short last block closing its call."""
        calls = []
        multi = self.channels_cap > 0 and res <= self.trials_cap
        cap = self._blocks_per_call(res) if multi else 1
        for i in ids:
            blk = i // res
            if calls:
                e0, E, b0, G = calls[-1]
                last = b0 + G - 1
                if i == e0 + E and blk == last and (multi or E < self.trials_cap):
                    calls[-1] = (e0, E + 1, b0, G)
                    continue
                if multi and i == e0 + E and blk == last + 1 and i % res == 0 and E == G * res and G < cap:
                    calls[-1] = (e0, E + 1, b0, G + 1)
                    continue
            calls.append((i, 1, blk, 1))
        return calls

    def _group_synth(self, SNR: float, ids: list, res: int):
        """The epochs `ids` (this rank's, in order) with every call's inputs drawn by TrialSynth: one
        launch for the call's channels (kept while the next call continues the same block), one for
        its trials, then forward_trials on the stacks.  Yields the epochs' Losses in order."""
        point = self._point << 32
        held = None                                   # (block, W, A [1, n, N], At, VAMP: (U, s, Vh))
        for e0, E, b0, G in self._synth_calls(ids, res):
            if G == 1 and held is not None and held[0] == b0:
                _, W, A, At, svd = held
            else:
                W, A, At = self.synth.channels(G, point + b0)
                svd = self._svd_gram(A) if self.detector == 'vamp' else None
                held = (b0, W, A, At, svd) if G == 1 else None
            x, sym, idx, y = self.synth.trials(At, E, res if G > 1 else E, SNR, point + e0)
            per = {'per_channel': res} if G > 1 else {}
            if self.detector == 'vamp':
                ch = svd if G > 1 else tuple(f[0] for f in svd)
            else:
                ch = ((W,) if self.detector == 'scamp' else ()) + ((A,) if G > 1 else (A[0],))
            yield from self.amp.forward_trials(*ch, y, SNR, x, sym, idx, **per)

    def _svd_gram(self, A):
        # the default keeps calling svd_gram(A) exactly as before (tools replace it by a one-argument function)
        return svd_gram(A) if self.device_svd == 'eigh' else svd_gram(A, method=self.device_svd)

    def _per_epoch_channels(self) -> bool:
        """Whether one launch may hold epochs with different channels (VAMP.epochs_channels_eligible)."""
        if self._ch_ok is None:
            n, N = self.config.Nr * self.config.Lout, self.config.Nt * self.config.Lin
            self._ch_ok = self.amp.epochs_channels_eligible(min(n, N))
        return self._ch_ok

    def _inputs(self, SNR: float, new_channel: bool):
        if new_channel:
            W, A = self.channel.generate_as_sparc()
            self._A = A
            self._W = W
            if self.detector == 'vamp':
                if self.rng == 'device':
                    self._svd = self._svd_gram(A)
                else:   # LAPACK on the host, as the reference's CPU path (vamp_model.py:58)
                    U, s, Vh = torch.linalg.svd(A.cpu(), full_matrices=False)
                    self._svd = (U.to(A.device), s.to(A.device), Vh.to(A.device))
        x, sym, idx = self.data.generate_message()
        if self.rng == 'device':
            # one [B, N] x [N, n] GEMM (torch's batched A @ x over [B, N, 1] runs as B GEMVs:
            # 2.5 ms at cfg4 on the box, r01)
            B = x.shape[0]
            y = (x.reshape(B, -1) @ self._A.transpose(0, 1)).reshape(B, -1, 1) + self.channel.awgn(SNR)
        else:
            # y = A x + n on the host as the reference's CPU path forms it (vamp_model.py:60)
            A_h = self._A if self._A.device.type == 'cpu' else self._A.cpu()
            y = (A_h @ x.cpu() + self.channel.awgn(SNR).cpu()).to(x.device)
        return x, sym, idx, y

    @torch.no_grad()
    def run(self, SNR: float) -> Loss:
        loss = self._epoch(SNR, True)
        print(loss.loss)
        return loss

    def _merge(self) -> None:
        """Sum the per-rank accumulated metrics (one all-reduce per SNR point).  Trial sharding
        needs none: every rank's Loss already holds the whole batch's counters."""
        if self.world == 1 or self.shard == 'trials':
            return
        keys = ['T'] + [k for k in self.loss.keys if k in self.loss.loss]
        vals = torch.tensor([float(np.asarray(self.loss.loss.get(k, 0.0), dtype=np.float64)) for k in keys],
                            dtype=torch.float64).to(_comm_device())
        torch.distributed.all_reduce(vals)
        vals = vals.cpu().numpy()
        self.loss.loss['T'] = float(vals[0])
        for k, v in zip(keys[1:], vals[1:]):
            self.loss.loss[k] = np.float64(v)

    @torch.no_grad()
    def simulate(self, epochs: int, final=None, start=None, step: float = 1, res: int = 1):
        if start is None:
            start = int(np.ceil(self.min_snr))
        if final is None:
            final = start + 20.0
        EbN0dB_range = np.arange(start, final + step, step)
        SNRdB_range = EbN0dB_range + 10 * np.log10(self.rate)
        results = []
        for self._point, (SNRdB, EbN0dB) in enumerate(zip(SNRdB_range, EbN0dB_range)):
            if self.rank == 0:
                print(f'EbN0dB={EbN0dB}')
            SNR = 10 ** (SNRdB / 10)
            # blocks of `res` epochs share a channel and go to one rank
            mine = [i for i in range(epochs) if (i // res) % self._epoch_world == self.rank % self._epoch_world]
            if self.group_cap > 1:
                for loss in self._group(SNR, mine, res):      # side by side, chunks of group_cap epochs
                    self.loss.accumulate(loss)
            elif self.synth is not None:
                for loss in self._group_synth(SNR, mine, res):    # inputs drawn per call on the device
                    self.loss.accumulate(loss)
            elif self.trials_cap > 0 and self.channels_cap > 0:
                for loss in self._group_trial_channels(SNR, mine, res):   # several channels per call
                    self.loss.accumulate(loss)
            elif self.trials_cap > 0:
                for loss in self._group_trials(SNR, mine, res):   # independent trials per channel run
                    self.loss.accumulate(loss)
            else:
                for i in mine:
                    loss = self._epoch(SNR, i % res == 0)
                    self.loss.accumulate(loss)
            if 'fer' not in self.loss.loss:                   # a rank without epochs at this point
                for k in self.loss.keys:
                    self.loss.loss[k] = np.float64(0.0)
            self._merge()
            self.loss.average(epochs)
            fer = self.loss.loss['fer']
            it = self.loss.loss['T']
            point = {k: (float(v) if np.ndim(v) == 0 else v) for k, v in self.loss.loss.items()}
            point.update(EbN0dB=float(EbN0dB), SNRdB=float(SNRdB))
            results.append(point)
            if self.rank == 0:
                print(f'FER={fer}, iter={it}')
                self.loss.export(SNRdB, EbN0dB, self.path)   # also clears the totals (loss.py:323)
            else:
                # every other rank clears its totals too (both shard modes): its next point must
                # start from zero, or its FER (and with it the stop decision below, which every
                # rank takes on the same merged / whole-batch values) would drift from rank 0's
                self.loss.loss = {'T': 0}
            if fer < 1e-3:
                break
        return results
