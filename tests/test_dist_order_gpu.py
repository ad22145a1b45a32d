"""The gradient exchange must be ordered behind every gradient it packs (fusiontransformer_amd/dist.py), also when a gradient is
late, arrives after its bucket's tail, or is produced on a stream the reducer has not seen before.

A missing wait is made CERTAIN to show: a pass-through autograd node whose backward spins the producing stream for a calibrated
100 ms sits in front of the producers of the late gradients, so a pack that does not wait for them copies the buffer before it has
been written (every step uses a fresh random input: whatever the buffer held differs from the expected gradient).  Each scenario
also records an event behind the delayed producers and requires it to be still pending when finish() returns -- otherwise the
delay did not cover the pack and the scenario would have proved nothing.

Streams share hardware queues (HIP gives a process four by default), and a queue's own order would hide the race: the delayed
stream is chosen by a probe (`_pick_stream`) so that work on the stream that packs really overtakes it.

The model is four (or six) bias-free Linear(64, 64); two weights fill a bucket; the twin is the same layers without a reducer.
The order of arrival is fixed by one backward() per layer.  All gradients are compared with torch.equal."""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

DELAY_MS = 100.0                           # two orders of magnitude above the host's path from a tail hook to the enqueued pack
BUCKET_MB = 2 * 64 * 64 * 4 / 2 ** 20      # exactly two 64x64 fp32 weights


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _timed_sleep(cycles):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(cycles)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _calibrate(ms=DELAY_MS):
    """Cycles of torch.cuda._sleep that last `ms` on this device: one timed sleep after a warm-up call, scaled, and measured again."""
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    probe = 1_000_000
    t = _timed_sleep(probe)
    while t < 2.0 and probe < 10 ** 11:       # long enough to time, whatever clock the spin kernel counts
        probe *= 10
        t = _timed_sleep(probe)
    cycles = int(probe * ms / t)
    got = _timed_sleep(cycles)
    assert got >= 0.9 * ms, "calibrated delay lasts %.1f ms, wanted %.0f" % (got, ms)
    return cycles


def _overtakes(waiter, delayed, cycles, scratch):
    """True when a kernel on `waiter` completes while a sleep issued before it on `delayed` is still running."""
    torch.cuda.synchronize()
    with torch.cuda.stream(delayed):
        torch.cuda._sleep(cycles)
        ev_d = torch.cuda.Event()
        ev_d.record()
    with torch.cuda.stream(waiter):
        scratch.add_(1)
        ev_w = torch.cuda.Event()
        ev_w.record()
    ev_w.synchronize()
    free = not ev_d.query()
    torch.cuda.synchronize()
    return free


def _pick_stream(waiters, cycles):
    """A new stream that does not hold up any of `waiters` (it shares no hardware queue with them)."""
    scratch = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(12):
        st = torch.cuda.Stream()
        if all(_overtakes(w, st, cycles // 5, scratch) for w in waiters):
            return st
    raise AssertionError("no stream found that leaves the packing stream free to run ahead: the delay could not expose a missing wait")


def _delay(cycles):
    class _Delay(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, g):
            torch.cuda._sleep(cycles)        # on the current stream: the one the forward ran on
            return g
    return _Delay.apply


def _layers(pairs):
    names = [k + str(i + 1) for i in range(pairs) for k in "ab"]      # a1 b1 a2 b2 ...
    return torch.nn.ModuleDict({n: torch.nn.Linear(64, 64, bias=False) for n in names}).cuda()


class _Rig:
    """Model + twin + reducer; `step` runs one training step's backward in a given order of arrival."""

    def __init__(self, pairs, cycles, stream, **reducer_args):
        from fusiontransformer_amd.dist import GradReducer
        self.model, self.twin = _layers(pairs), _layers(pairs)
        self.twin.load_state_dict(self.model.state_dict())
        self.names = list(self.model.keys())
        self.red = GradReducer(self.model, bucket_mb=BUCKET_MB, **reducer_args)
        self.delay, self.stream = _delay(cycles), stream

    def losses(self, mods, x, delayed=None):
        out = {}
        for n in self.names:
            y = mods[n](x)
            if n == delayed:
                y = self.delay(y)            # its backward runs BEFORE the layer's: the sleep is queued in front of the producer
            out[n] = y.pow(2).sum()
        return out

    def step(self, order, delayed=None, stream=None, join=False):
        """-> (the event behind the delayed producers was still pending when finish() returned, names of the wrong gradients)"""
        stream = stream or self.stream
        x = torch.randn(32, 64, device="cuda")
        self.twin.zero_grad(set_to_none=True)
        ref = self.losses(self.twin, x)
        for n in order:
            ref[n].backward()
        torch.cuda.synchronize()
        self.red.begin_step()
        with torch.cuda.stream(stream):
            losses = self.losses(self.model, x, delayed)
            for n in order:
                losses[n].backward()
            behind = torch.cuda.Event()
            behind.record()
            if not join:
                self.red.finish()
        if join:
            torch.cuda.current_stream().wait_stream(stream)
            self.red.finish()
        pending = not behind.query()
        torch.cuda.synchronize()
        bad = [n for n in self.names if self.model[n].weight.grad is None or not torch.equal(self.model[n].weight.grad, self.twin[n].weight.grad)]
        return pending, bad

    def warm_up(self):
        """Step 0 records the order, step 1 rebuilds the buckets (and pays RCCL's lazy set-up) -> early launches of step 1."""
        pairs = len(self.names) // 2
        assert self.step(self.names)[1] == []
        assert self.step(self.names)[1] == []
        name_of = {id(m.weight): n for n, m in self.model.items()}
        got = [[name_of[id(p)] for p in b.params] for b in self.red.buckets]
        assert self.red._rebuilt and got == [["a%d" % (i + 1), "b%d" % (i + 1)] for i in range(pairs)], got
        return self.red.hook_stats["early_launches"]


def _order_worker(port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
        import torch.distributed as dist
        torch.cuda.set_device(0)
        from fusiontransformer_amd.dist import init_process_group
        init_process_group("nccl", force=True)
        assert dist.is_initialized() and dist.get_backend() == "nccl" and dist.get_world_size() == 1
        torch.manual_seed(11)
        cycles = _calibrate()
        res = {}

        two = _Rig(2, cycles, None, force_collectives=True)
        comm = two.red._comm_stream(torch.device("cuda", 0))       # the exchange stream (every reducer of the process uses its own)
        with torch.cuda.stream(comm):
            torch.zeros(1, device="cuda")                          # first use: the stream gets its hardware queue now
        two.stream = _pick_stream([comm], cycles)
        early1 = two.warm_up()
        assert early1 >= 1, early1
        # S1: the b losses go backward first (both tails fire, bucket 0 incomplete at its own), then the delay, then the a losses;
        # bucket 0 goes out from finish()
        deferred = two.red.hook_stats["deferred"]
        res["S1"] = two.step(["b1", "b2", "a1", "a2"], delayed="a1") + (two.red.hook_stats["deferred"] - deferred,)
        # S2: the recorded order, everything on a stream created after step 0; bucket 0 goes out early, from bucket 1's tail
        s_new = _pick_stream([comm], cycles)
        early = two.red.hook_stats["early_launches"]
        res["S2"] = two.step(two.names, delayed="a1", stream=s_new, join=True) + (two.red.hook_stats["early_launches"] - early,)
        # S3: back to normal; the overlap is still on
        early = two.red.hook_stats["early_launches"]
        res["S3"] = two.step(two.names) + (two.red.hook_stats["early_launches"] - early, early1)

        # S1b: three buckets; bucket 0 is incomplete at its tail, a1 arrives late, and bucket 0 goes out from bucket 1's tail
        three = _Rig(3, cycles, None, force_collectives=True, broadcast_params=False)
        comm3 = three.red._comm_stream(torch.device("cuda", 0))
        with torch.cuda.stream(comm3):
            torch.zeros(1, device="cuda")
        three.stream = _pick_stream([comm3], cycles)
        three.warm_up()
        early = three.red.hook_stats["early_launches"]
        res["S1b"] = three.step(["b1", "a1", "a2", "b2", "a3", "b3"], delayed="a1") + (three.red.hook_stats["early_launches"] - early,)
        q.put(("ok", res))
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put(("error", traceback.format_exc()))
        raise


@pytest.fixture(scope="module")
def active():
    """The active-path scenarios, run once in one child process over a one-rank RCCL communicator."""
    import multiprocessing as mp
    import queue
    ctx = mp.get_context("forkserver")
    q = ctx.Queue()
    p = ctx.Process(target=_order_worker, args=(_free_port(), q))
    p.start()
    try:
        status, res = q.get(timeout=300)
    except queue.Empty:
        status, res = "error", "the child reported nothing within 300 s"
    p.join(timeout=60)
    if p.is_alive():
        p.terminate()
        p.join(timeout=30)
        status, res = "error", "the child did not exit; it had reported: %r" % (res,)
    assert status == "ok", "the child failed:\n%s" % res
    assert p.exitcode == 0, p.exitcode
    return res


def _check(pending, bad):
    assert pending, "the delayed producers had already run when finish() returned: the delay did not cover the pack, nothing was proved"
    assert bad == [], "gradients differ from the twin's (packed before their producer had written them): %s" % bad


def test_late_gradient_of_a_bucket_sent_from_finish_is_waited_for(active):
    pending, bad, deferred = active["S1"]
    _check(pending, bad)
    assert deferred >= 1, deferred


def test_late_gradient_of_a_bucket_sent_from_a_later_tail_is_waited_for(active):
    pending, bad, early = active["S1b"]
    _check(pending, bad)
    assert early >= 1, "no bucket went out from a tail hook: bucket 0 was meant to leave from bucket 1's tail"


def test_gradients_of_a_stream_first_seen_after_step_0_are_waited_for(active):
    pending, bad, early = active["S2"]
    _check(pending, bad)
    assert early >= 1, "bucket 0 was meant to go out early, from bucket 1's tail"


def test_unchanged_order_afterwards_is_exact_and_still_overlaps(active):
    _, bad, early, early1 = active["S3"]
    assert bad == [], bad
    assert early == early1 and early1 >= 1, (early, early1)


def test_inactive_reducer_never_reads_the_other_streams_gradients_unordered():
    """World size 1, no collectives: the a layers (delayed) run on one stream, the b layers on another, one backward over the sum.
    Bucket 0 holds the a gradients and bucket 1's tail is a b gradient, so a pack issued from that tail's hook would run on the b
    stream, ahead of the a stream."""
    import torch.distributed as dist
    from fusiontransformer_amd.dist import GradReducer
    assert not dist.is_initialized()
    torch.manual_seed(12)
    cycles = _calibrate()
    model, twin = _layers(2), _layers(2)
    twin.load_state_dict(model.state_dict())
    red = GradReducer(model, bucket_mb=BUCKET_MB)
    assert not red.active
    delay = _delay(cycles)
    sb = torch.cuda.Stream()
    with torch.cuda.stream(sb):
        torch.zeros(1, device="cuda")
    sa = _pick_stream([sb, torch.cuda.current_stream()], cycles)

    def total(mods, x, delayed, with_b, streams):
        cur = torch.cuda.current_stream()
        parts = []
        if with_b:                              # created first -> goes backward last
            with torch.cuda.stream(streams[1]):
                lb = mods["b1"](x).pow(2).sum() + mods["b2"](x).pow(2).sum()
            cur.wait_stream(streams[1])
            parts.append(lb)
        with torch.cuda.stream(streams[0]):
            la = mods["a1"](x).pow(2).sum() + mods["a2"](x).pow(2).sum()
            la = delay(la) if delayed else la    # in front of the whole a branch's backward
        cur.wait_stream(streams[0])
        parts.append(la)
        return sum(parts)

    def step(delayed=False, with_b=True):
        x = torch.randn(32, 64, device="cuda")
        twin.zero_grad(set_to_none=True)
        cur = torch.cuda.current_stream()
        total(twin, x, False, with_b, (cur, cur)).backward()
        torch.cuda.synchronize()
        red.begin_step()
        loss = total(model, x, delayed, with_b, (sa, sb))
        loss.backward()
        behind = torch.cuda.Event()
        behind.record(sa)
        red.finish()
        pending = not behind.query()
        torch.cuda.synchronize()
        return pending

    def wrong(names):
        return [n for n in names if model[n].weight.grad is None or not torch.equal(model[n].weight.grad, twin[n].weight.grad)]

    every = ["a1", "b1", "a2", "b2"]
    for _ in range(2):
        step()
        assert wrong(every) == []
    a_weights = {id(model["a1"].weight), id(model["a2"].weight)}
    assert red._rebuilt and len(red.buckets) == 2 and {id(p) for p in red.buckets[0].params} == a_weights and \
        id(red.buckets[1].params[-1]) not in a_weights, "the buckets are not the ones this scenario is about"
    _check(step(delayed=True), wrong(every))
    assert all(model[n].weight.grad.data_ptr() % 16 == 0 for n in every)      # what ftx_adam_step's vector loads need
    # a parameter that got no gradient this step ends with zeros, not None
    step(with_b=False)
    assert wrong(["a1", "a2"]) == []
    for n in ("b1", "b2"):
        g = model[n].weight.grad
        assert g is not None and g.shape == model[n].weight.shape and not g.any().item(), n
