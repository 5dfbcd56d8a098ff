"""Readers for the reference-generated golden fixtures in tests/golden/ (data only)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


class Case(dict):
    def __getattr__(self, k):
        return self[k]


def _group(npz):
    out = {}
    for k in npz.files:
        if '/' not in k:
            continue
        key, field = k.split('/', 1)
        out.setdefault(key, Case())[field] = npz[k]
    return out


PART_LIMIT = 1000000     # no committed file is larger than 1 MiB; this leaves a margin


class Parts:
    """The arrays of tests/golden/<stem>.part<k>.npz, k = 0, 1, ..., read like one npz file: a
    fixture that would be larger than PART_LIMIT in one file is stored in parts (save_parts)."""

    def __init__(self, stem):
        self._of = {}
        k = 0
        while os.path.exists(os.path.join(GOLDEN, f'{stem}.part{k}.npz')):
            z = np.load(os.path.join(GOLDEN, f'{stem}.part{k}.npz'))
            for name in z.files:
                assert name not in self._of, (stem, name)
                self._of[name] = z
            k += 1
        if not k:
            raise FileNotFoundError(os.path.join(GOLDEN, f'{stem}.part0.npz'))
        self.files = list(self._of)

    def __getitem__(self, name):
        return self._of[name][name]


def save_parts(stem, flat, limit=PART_LIMIT):
    """Writes the arrays `flat` ('<case>/<field>': array) as tests/golden/<stem>.part<k>.npz, each
    at most `limit` bytes: whole cases in their given order, a new part begun when the next case
    would take the current one over the limit.  Removes the parts of an earlier, longer run."""
    import io
    cases = {}
    for name, a in flat.items():
        cases.setdefault(name.split('/', 1)[0], {})[name] = a

    def packed(arrays):
        buf = io.BytesIO()
        np.savez_compressed(buf, **arrays)
        return buf.getvalue()

    parts, cur = [], {}
    for arrays in cases.values():
        if cur and len(packed({**cur, **arrays})) > limit:
            parts.append(cur)
            cur = {}
        cur.update(arrays)
    parts.append(cur)
    for k, arrays in enumerate(parts):
        raw = packed(arrays)
        assert len(raw) <= limit, (stem, k, len(raw))
        with open(os.path.join(GOLDEN, f'{stem}.part{k}.npz'), 'wb') as f:
            f.write(raw)
    k = len(parts)
    while os.path.exists(os.path.join(GOLDEN, f'{stem}.part{k}.npz')):
        os.remove(os.path.join(GOLDEN, f'{stem}.part{k}.npz'))
        k += 1
    return len(parts)


def g1_cases():
    """{name: Case} — per-iteration reference traces with their stored inputs."""
    cases = _group(Parts('g1_traces'))
    for name, c in cases.items():
        algo, alph, ebn0, seed = name.split('_')
        c['algo'], c['alphabet'], c['EbN0'], c['seed'] = algo, alph, float(ebn0), int(seed)
        c['loss_ref'] = json.loads(str(c['loss']))
    return cases


def g12_cases():
    """{name: Case} — vamp2.py (damped VAMP) reference traces with their stored inputs."""
    cases = _group(np.load(os.path.join(GOLDEN, 'g12_vamp2.npz')))
    for name, c in cases.items():
        _, alph, nt, ebn0, seed, damp = name.split('_')
        c['alphabet'], c['EbN0'], c['seed'] = alph, float(ebn0), int(seed)
        c['loss_ref'] = json.loads(str(c['loss']))
    return cases


def g2_cases():
    return _group(np.load(os.path.join(GOLDEN, 'g2_denoiser.npz')))


def g3_cases():
    cases = _group(np.load(os.path.join(GOLDEN, 'g3_decision.npz')))
    for c in cases.values():
        c['loss_ref'] = json.loads(str(c['loss']))
    return cases


def g4_curves():
    with open(os.path.join(GOLDEN, 'g4_curves.json')) as f:
        return json.load(f)


LOSS_KEYS = ['fer', 'nMSE', 'nMSEf', 'nMSEm', 'nMSEL', 'ver', 'verf', 'verm', 'verL', 'ber', 'iber', 'sber',
             'ier', 'ser']
COUNT_KEYS = ['fer', 'ver', 'verf', 'verm', 'verL', 'ber', 'iber', 'sber', 'ier', 'ser']


def loss_close(got: dict, ref: dict, count_tol=0.0, mse_rtol=1e-3):
    """Compare Loss dicts: counting metrics within `count_tol` absolute, nMSE* within mse_rtol."""
    bad = {}
    for k in LOSS_KEYS:
        g, r = float(np.asarray(got[k])), float(ref[k])
        if np.isnan(r) or np.isnan(g):
            if not (np.isnan(r) and np.isnan(g)):
                bad[k] = (g, r)
            continue
        if k.startswith('nMSE'):
            if abs(g - r) > mse_rtol * max(abs(r), 1e-12) + 1e-9:
                bad[k] = (g, r)
        elif abs(g - r) > count_tol + 1e-12:
            bad[k] = (g, r)
    return bad


def bits_equal(a, b) -> bool:
    """Bitwise equality of two device tensors (NaN payloads included): the NaN-onset iterations
    must agree too, which torch.equal (NaN != NaN) cannot check."""
    import torch
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    w = torch.int64 if a.element_size() == 8 else torch.int32
    return torch.equal(a.contiguous().view(w), b.contiguous().view(w))
