"""A trial-sharded VAMP forward inside ONE process (test_gpu_vamp_wide.py,
test_gpu_vamp_launch_iter.py): the slices of one batch are detected by threads whose all-reduce hook
meets on a barrier.  The barrier has a timeout and a failed thread aborts it, so a failure ends the
test instead of hanging it."""
import threading

import torch


class Exchange:
    """The all-reduce of the slices detected by the threads of one process: each thread's hook puts
    its float64 words on the host, the threads meet, each takes the reduction of all."""

    def __init__(self, world):
        self.local = threading.local()
        self.barrier = threading.Barrier(world, timeout=60)
        self.slots = [None] * world

    def allreduce(self, buf, count, op):
        import amp_native as nat
        ws = self.local.det._ws
        off = int(buf) - ws.data_ptr()
        assert 0 <= off and off + 8 * count <= ws.numel()
        view = ws[off:off + 8 * count].view(torch.float64)
        self.slots[self.local.rank] = view.cpu()           # after the slice's launches on its stream
        self.barrier.wait()
        both = torch.stack(self.slots)
        tot = both.sum(0) if op == nat.ALLREDUCE_SUM else torch.where(torch.isnan(both).any(0), both.sum(0),
                                                                      both.max(0).values)
        self.barrier.wait()                                # all have read the slots
        view.copy_(tot)


def run_slices(monkeypatch, make_config, inp, collect, rows: int = 24, world: int = 2):
    """ShardedVAMP over `world` slices of `rows` trials each, one thread per slice, on the whole
    batch's inputs `inp` (U, s, Vh, y, SNR, x, sym, idx on the device).  make_config() -> the batch's
    Config; collect(det, L) -> what the slice's thread returns (called on that thread, after its
    forward).  Returns the slices' results in rank order; asserts that no thread raised."""
    import amp_native as nat
    from vamp import ShardedVAMP
    xch = Exchange(world)
    workspace_type = type(nat.WORKSPACE)

    class PerThreadWorkspace:                              # one workspace cache per slice
        def get(self, dev, key, nbytes):
            if not hasattr(xch.local, 'ws'):
                xch.local.ws = workspace_type()
            return xch.local.ws.get(dev, key, nbytes)

    monkeypatch.setattr(nat, 'WORKSPACE', PerThreadWorkspace())

    class Slice(ShardedVAMP):
        bounds = (0, 0)

        def shard(self):
            return self.bounds

        def _allreduce(self, buf, count, op, stream, ctx):
            try:
                xch.allreduce(buf, count, op)
                return 0
            except Exception as e:   # noqa: BLE001 — reported by _run_hooked
                self._hook_error = self._hook_error or e
                return 1

    out, errs = [None] * world, []

    def run(rank):
        try:
            with torch.cuda.device(inp['y'].device):
                det = Slice(make_config())
                det.bounds = (rows * rank, rows * rank + rows)
                xch.local.rank, xch.local.det = rank, det
                L = det(inp['U'], inp['s'], inp['Vh'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
                out[rank] = collect(det, L)
        except Exception as e:   # noqa: BLE001
            errs.append((rank, repr(e)))
            xch.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    return out
