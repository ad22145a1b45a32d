"""world_size-2 gloo test of the gradient reducer (the N>1 path of bench.py) on the CPU."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from fusiontransformer_amd.dist import GradReducer, init_process_group
    r, w, _ = init_process_group("gloo")
    assert (r, w) == (rank, world)
    torch.manual_seed(100 + rank)   # different initial weights per rank: the reducer must broadcast rank 0's
    model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))
    for p in model[4].parameters():
        pass
    frozen = torch.nn.Linear(4, 4)           # never used: must not break the exchange
    for p in frozen.parameters():
        p.requires_grad_(False)
    model.add_module("frozen", frozen)
    red = GradReducer(model, bucket_mb=0.0005)   # tiny buckets -> several all-reduces, order matters
    w0 = [p.detach().clone() for p in model.parameters()]
    gathered = [torch.zeros_like(w0[0]) for _ in range(world)]
    dist.all_gather(gathered, w0[0])
    assert all(torch.equal(g, gathered[0]) for g in gathered), "parameters not broadcast"
    # a twin without the reducer yields this rank's purely local gradients (once buckets overlap
    # with the backward, p.grad of the reduced model is already averaged when backward returns)
    twin = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))
    twin.load_state_dict({k: v for k, v in model.state_dict().items() if not k.startswith("frozen")})
    ok = True
    for step in range(4):
        torch.manual_seed(1000 + 10 * step + rank)
        x = torch.randn(5, 8)
        twin.zero_grad()
        twin(x).pow(2).sum().backward()
        local = [p.grad.detach().clone() for p in twin.parameters()]
        red.begin_step()
        loss = model[:5](x).pow(2).sum()
        loss.backward()
        red.finish()
        # reference: average of the per-rank local gradients
        for p, g_local in zip([p for p in model.parameters() if p.requires_grad], local):
            parts = [torch.zeros_like(g_local) for _ in range(world)]
            dist.all_gather(parts, g_local)
            ref = sum(parts) / world
            ok = ok and torch.allclose(p.grad, ref, atol=1e-6)
    q.put((rank, ok, red._rebuilt, len(red.buckets)))
    dist.barrier()
    dist.destroy_process_group()


def test_grad_reducer_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok, rebuilt, nb in res:
        assert ok, f"rank {rank}: reduced gradients differ from the average of the local ones"
        assert rebuilt and nb > 1


def _forced_worker(port, q):
    """World size 1 with the collective path forced on: the all-reduce of one rank is the identity, so the reduced gradients must be the
    local ones to the last bit, and every bucket must have gone through a collective."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    from fusiontransformer_amd.dist import GradReducer, init_process_group
    with pytest.raises(RuntimeError):
        GradReducer(torch.nn.Linear(2, 2), force_collectives=True)      # no process group yet
    r, w, _ = init_process_group("gloo", force=True)
    assert (r, w) == (0, 1) and dist.is_initialized()
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))
    twin = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))
    twin.load_state_dict(model.state_dict())
    red = GradReducer(model, bucket_mb=0.0005, force_collectives=True)
    assert red.active and GradReducer(twin).active is False
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    ok = True
    for step in range(3):
        x = torch.randn(5, 8)
        twin.zero_grad()
        twin(x).pow(2).sum().backward()
        red.begin_step()
        model(x).pow(2).sum().backward()
        red.finish()
        ok = ok and all(torch.equal(p.grad, t.grad) for p, t in zip(model.parameters(), twin.parameters()))
    dist.all_reduce = real
    q.put((ok, len(calls), len(red.buckets), red._rebuilt))
    dist.destroy_process_group()


def test_forced_collectives_at_world_size_one():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_forced_worker, args=(_free_port(), q))
    p.start()
    ok, calls, nb, rebuilt = q.get(timeout=120)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert ok, "a one-rank all-reduce changed the gradients"
    assert nb > 1 and rebuilt and calls >= 3 * nb, (calls, nb)


def _reorder_worker(port, q):
    """From step 1 only the last-ready parameter of each bucket keeps a hook.  If the gradient-ready ORDER changes in a later step -- the
    tail fires while another gradient of its bucket is still missing -- the bucket must not go out early: it waits for finish()."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    from fusiontransformer_amd.dist import GradReducer, init_process_group
    init_process_group("gloo", force=True)
    torch.manual_seed(4)
    a, b = torch.nn.Linear(6, 6), torch.nn.Linear(6, 6)
    model = torch.nn.ModuleList([a, b])
    red = GradReducer(model, bucket_mb=1e-9, force_collectives=True)      # one parameter per bucket
    x = torch.randn(3, 6)

    def step(order):
        red.begin_step()
        outs = {"a": a(x).pow(2).sum(), "b": b(x).pow(2).sum()}
        for name in order:                       # two separate backward calls fix the order in which the gradients arrive
            outs[name].backward()
        red.finish()
        return [p.grad.clone() for p in model.parameters()]

    g0 = step("ab")
    g1 = step("ab")                              # buckets rebuilt in the recorded order, one hook per bucket
    early = red.hook_stats["early_launches"]
    g2 = step("ba")                              # the order flips: nothing may go out before its bucket is complete
    ok = all(torch.equal(u, v) for u, v in zip(g0, g1)) and all(torch.equal(u, v) for u, v in zip(g0, g2))
    q.put((ok, red._rebuilt, len(red.buckets), early, red.hook_stats["deferred"]))
    dist.destroy_process_group()


def test_bucket_waits_when_the_gradient_order_changes():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_reorder_worker, args=(_free_port(), q))
    p.start()
    ok, rebuilt, nb, early, deferred = q.get(timeout=120)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert ok, "gradients changed when the ready order changed"
    assert rebuilt and nb == 4 and early >= 1 and deferred >= 1, (nb, early, deferred)


# ---- the ordering contract of the exchange, stated without timing -------------------------------------------------------------------
# Every pack of a bucket is preceded by a mark of that bucket made after the last of its gradients arrived, and that mark covers
# every stream a gradient of the step was accumulated on; a pack issued from a hook (before finish()) needs a mark at which the bucket
# was complete.  GradReducer marks (_mark), packs (_pack) and learns streams (_note_stream) through small methods called on every
# device, so a subclass can log them on the CPU, with pretend streams.  tests/test_dist_order_gpu.py shows the same on the GPU.

def _contract_worker(port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    from fusiontransformer_amd.dist import GradReducer, init_process_group
    init_process_group("gloo", force=True)
    torch.manual_seed(6)

    class Logged(GradReducer):
        log, now = None, "s0"                    # `now`: the pretend current stream

        def _state(self, b):
            return (self.buckets.index(b), tuple(p.grad is not None for p in b.params), frozenset(self._streams))

        def _note_stream(self, device):
            self._streams[self.now] = self.now

        def _mark(self, b):
            super()._mark(b)
            self.log.append(("mark",) + self._state(b) + (b.complete,))

        def _pack(self, b, early=False):
            state = self._state(b)
            done = super()._pack(b, early)
            if done:
                self.log.append(("pack",) + state)
            return done

        def finish(self):
            self.log.append(("finish",))
            super().finish()

    def rig(pairs, **kw):
        names = [k + str(i + 1) for i in range(pairs) for k in "ab"]
        model = torch.nn.ModuleDict({n: torch.nn.Linear(6, 6, bias=False) for n in names})
        twin = torch.nn.ModuleDict({n: torch.nn.Linear(6, 6, bias=False) for n in names})
        twin.load_state_dict(model.state_dict())
        log = []
        for n in names:                           # registered before the reducer's hooks: an arrival is logged before the mark it causes
            model[n].weight.register_post_accumulate_grad_hook(lambda p, n=n: log.append(("grad", n, red.now)))
        red = Logged(model, bucket_mb=2 * 36 * 4 / 2 ** 20, **kw)     # two weights fill a bucket
        red.log = log

        def step(order, stream="s0"):
            """-> (this step's log, bucket of every layer, names whose gradient differs from the twin's; a layer left out of
            `order` must end with zeros)"""
            del log[:]
            red.now = stream
            x = torch.randn(3, 6)
            twin.zero_grad(set_to_none=True)
            red.begin_step()
            for n in order:
                twin[n](x).pow(2).sum().backward()
                model[n](x).pow(2).sum().backward()
            red.now = "s0"                        # the caller's stream
            red.finish()
            want = {n: twin[n].weight.grad if n in order else torch.zeros(6, 6) for n in names}
            bad = [n for n in names if model[n].weight.grad is None or not torch.equal(model[n].weight.grad, want[n])]
            where = {n: i for i, b in enumerate(red.buckets) for n in names if any(model[n].weight is p for p in b.params)}
            return list(log), where, bad
        step(names)
        step(names)
        assert red._rebuilt and [len(b.params) for b in red.buckets] == [2] * pairs
        return names, step

    out = {}
    names, step = rig(2, force_collectives=True)
    out["unchanged"] = step(names)
    out["flipped, sent from finish"] = step(["b1", "b2", "a1", "a2"])
    out["new stream"] = step(names, stream="s1")
    out["no gradient"] = step(["a1", "b1", "a2"])
    names3, step3 = rig(3, force_collectives=True, broadcast_params=False)
    out["flipped, sent from a later tail"] = step3(["b1", "a1", "a2", "b2", "a3", "b3"])
    names1, step1 = rig(2)                        # no collectives: packs in finish() only
    out["inactive"] = step1(names1)
    out["inactive, no gradient"] = step1(["a1", "b1", "a2"])
    q.put(out)
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def contract_logs():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_contract_worker, args=(_free_port(), q))
    p.start()
    out = q.get(timeout=120)
    p.join(timeout=60)
    assert p.exitcode == 0
    return out


def _assert_contract(log, where, bad, active=True):
    """The contract, read off one step's log.  -> the buckets packed before finish(), in order."""
    assert bad == [], "gradients differ from the twin's: %s" % bad
    assert [e[0] for e in log].count("finish") == 1
    early, arrived, streams, last_mark, in_finish, packed = [], set(), set(), {}, False, []
    for e in log:
        if e[0] == "grad":
            arrived.add(e[1])
            streams.add(e[2])
        elif e[0] == "finish":
            in_finish = True
        elif e[0] == "mark":
            last_mark[e[1]] = (e, set(arrived), in_finish)
        else:
            _, i, present, known = e
            packed.append(i)
            members = {n for n, k in where.items() if k == i}
            assert sum(present) == len(members & arrived), (e, arrived)
            if not in_finish:
                early.append(i)
            if not active:
                assert in_finish, "a reducer without collectives packed bucket %d from a hook" % i
                continue
            assert i in last_mark, "bucket %d was packed without a mark" % i
            (_, _, seen, covered, complete), arrived_then, marked_in_finish = last_mark[i]
            assert members & arrived <= arrived_then, "bucket %d: %s arrived after the mark its pack waited for" % (i, sorted((members & arrived) - arrived_then))
            assert seen == present and complete == all(present)
            assert streams <= covered, "bucket %d: the mark does not cover stream(s) %s" % (i, sorted(streams - covered))
            if in_finish:
                assert marked_in_finish, "bucket %d went out from finish() behind a mark made earlier" % i
            else:
                assert complete, "bucket %d went out early behind a mark at which it was incomplete" % i
    assert packed == sorted(set(where.values())), "every bucket is packed once, in bucket order: %s" % packed
    return early


def test_contract_unchanged_order_overlaps_behind_the_tail_marks(contract_logs):
    log, where, bad = contract_logs["unchanged"]
    assert _assert_contract(log, where, bad) == [0]
    # the usual case costs nothing extra: bucket 0 is marked once, at its own tail, and goes out behind that mark
    assert [e[1] for e in log if e[0] == "mark"] == [0, 1, 1]


def test_contract_flipped_order_bucket_sent_from_finish(contract_logs):
    log, where, bad = contract_logs["flipped, sent from finish"]
    assert _assert_contract(log, where, bad) == []
    assert where["a1"] == where["b1"] == 0 and where["a2"] == where["b2"] == 1


def test_contract_flipped_order_bucket_sent_from_a_later_tail(contract_logs):
    log, where, bad = contract_logs["flipped, sent from a later tail"]
    # bucket 0 (incomplete at its tail, a1 late) leaves from bucket 1's tail behind a NEW mark; bucket 1 from bucket 2's tail
    assert _assert_contract(log, where, bad) == [0, 1]
    assert [e[1] for e in log if e[0] == "mark"][:3] == [0, 1, 0]


def test_contract_stream_first_seen_in_a_later_step_is_covered(contract_logs):
    log, where, bad = contract_logs["new stream"]
    assert _assert_contract(log, where, bad) == [0]
    assert all("s1" in e[3] for e in log if e[0] == "mark")


def test_contract_parameter_without_a_gradient(contract_logs):
    log, where, bad = contract_logs["no gradient"]
    # b2 is bucket 1's tail and never arrives: no hook fires after bucket 0's own tail, so both buckets leave from finish()
    assert _assert_contract(log, where, bad) == []
    assert [e[2] for e in log if e[0] == "pack"] == [(True, True), (True, False)]


def test_contract_reducer_without_collectives_packs_in_finish_only(contract_logs):
    for case in ("inactive", "inactive, no gradient"):
        log, where, bad = contract_logs[case]
        assert _assert_contract(log, where, bad, active=False) == []
        assert not [e for e in log if e[0] == "mark"]
