"""The one checker of the SPVCNN op program (csrc/ftx_spvcnn_program.h: check_program) as the eval executor (ftx_spvcnn_eval) and the
training executor (ftx_spvcnn_train_fwd / _bwd) apply it: the conditions they share refuse the same tables with the same text, and
the conditions that differ differ exactly as listed here.  The expected texts are those of the library before the two checkers
became one.  No GPU: every run call is given a null arena, so a table that is wrongly accepted is refused there and fails its
assertion instead of launching."""
import pytest
import torch

from fusiontransformer_amd import native_eval as ne
from fusiontransformer_amd import native_train as nt
from fusiontransformer_amd.models.spvcnn import SPVCNN
from tests import test_native_eval_host as eh
from tests import test_native_train_host as th

FTX_EINVAL = -1
KEYS = ("layers", "ops", "rows", "maps", "pvs", "routes", "groutes")
EVAL, TRAIN = "ftx_spvcnn_eval: ", "ftx_spvcnn_train: "
ARENA = "the arena must be a 256-byte aligned device buffer"       # what a run call answers once the program is accepted
# sites in the emitted program (the same op indices in the eval and the training program: they differ in the segment numbers alone)
STEM2, DEVOX, EXT, VOX, DOWN, CONV3, DENSE, LINEAR, ADD, EXT2, CONCAT, LAST_LINEAR, LAST = 1, 2, 3, 4, 5, 6, 11, 29, 30, 31, 34, 66, 67


@pytest.fixture(scope="module")
def programs():
    torch.manual_seed(0)
    net = SPVCNN()
    program, tp = ne.emit_program(net), nt.TrainProgram(net)
    ops = program.ops_array()
    assert [int(ops[i]["kind"]) for i in (STEM2, DEVOX, EXT, VOX, DOWN, CONV3, DENSE, LINEAR, ADD, EXT2, CONCAT, LAST_LINEAR, LAST)] == [
        ne.OP_CONV_BN, ne.OP_DEVOXELIZE, ne.OP_ADD_EXT, ne.OP_VOXELIZE, ne.OP_CONV_BN, ne.OP_CONV_BN, ne.OP_CONV_BN, ne.OP_LINEAR_BN, ne.OP_ADD,
        ne.OP_ADD_EXT, ne.OP_CONCAT, ne.OP_LINEAR_BN, ne.OP_ADD] and len(ops) == LAST + 1
    return program, tp


def both(programs, mutate=None, **kw):
    """The standard tables of the two host tests for the eval and the training program, after the same mutation of each."""
    program, tp = programs
    out = []
    for t in (eh.tables(program, **kw), th.train_tables(tp, **kw)):
        t = dict(zip(KEYS, t))
        if mutate is not None:
            mutate(t)
        out.append(tuple(t[k] for k in KEYS[:len(t)]))
    return out


def answers(ftx_lib, ev, tr):
    """[(size, text of the size query, rc of the run, text of the run)] of the eval executor, the training forward and the backward."""
    out = []
    for size, run in ((lambda: eh.size(ftx_lib, ev), lambda: eh.call(ftx_lib, ev, arena=None, arena_bytes=1 << 40)),
                      (lambda: th.size(ftx_lib, tr), lambda: th.call(ftx_lib, tr, "fwd", arena=None, arena_bytes=1 << 40)),
                      (lambda: th.size(ftx_lib, tr), lambda: th.call(ftx_lib, tr, "bwd", arena=None, arena_bytes=1 << 40))):
        n = size()
        text = ftx_lib.ftx_last_error().decode() if n == 0 else ""
        out.append((n, text) + run())
    return out


def refused(answer, text):
    n, size_text, rc, run_text = answer
    return n == 0 and rc == FTX_EINVAL and size_text == text and run_text == text


def accepted(answer):
    n, _, rc, run_text = answer
    return n > 0 and n % 256 == 0 and rc == FTX_EINVAL and ARENA in run_text


def setter(table, index, field, value):
    def mutate(t):
        t[table][index][field] = value
    return mutate


def set_rows(level, n):
    def mutate(t):
        t["rows"][level] = n
    return mutate


def set_route(op, route):
    def mutate(t):
        t["routes"][op] = route
    return mutate


def no_pairs(m, route_of=None, route=None, null=()):
    def mutate(t):
        t["maps"][m]["n_pairs"] = 0
        for f in null:
            t["maps"][m][f] = 0
        if route_of is not None:
            t["routes"][route_of] = route
    return mutate


# one mutation per condition the two executors share -> the text both give, after the entry's name
SHARED = [
    ("unknown kind", setter("ops", CONV3, "kind", 9), "op 6: unknown kind 9"),
    ("level out of range", setter("ops", CONV3, "level", 6), "op 6 (conv_bn): level 6"),
    ("channel count 6", setter("ops", CONV3, "channels", 6), "op 6 (conv_bn): channel count 6 is not a multiple of 4 in [4, 1024]"),
    ("channel count above 1024", setter("ops", CONV3, "channels", 1028), "op 6 (conv_bn): channel count 1028 is not a multiple of 4 in [4, 1024]"),
    ("layer index out of range", setter("ops", CONV3, "layer", 1000), "op 6 (conv_bn): layer 1000 out of range"),
    ("layer of the other kind", setter("ops", CONV3, "layer", 25), "op 6 (conv_bn): layer 25 is of another kind"),
    ("layer channels not a multiple of 4", setter("layers", 3, "co", 30), "op 6 (conv_bn) layer 3: channels must be multiples of 4 (ca=32 co=30)"),
    ("layer channels against the slots", setter("layers", 3, "ca", 64), "op 6 (conv_bn) layer 3: channel counts do not match the slots"),
    ("null parameter", setter("layers", 3, "gamma", 0), "op 6 (conv_bn) layer 3: null parameter"),
    ("dense layer with a pair route", set_route(LINEAR, ne.ROUTES["pairs"]), "op 29 (linear_bn) layer 25: a dense layer takes the rows route, got 3"),
    ("dense layer with a stride", setter("layers", 8, "stride", 2), "op 11 (conv_bn) layer 8: unsupported dense layer"),
    ("kvol 5", setter("layers", 3, "kvol", 5), "op 6 (conv_bn) layer 3: kernel volume 5 (1, 8 or 27)"),
    ("map index out of range", setter("ops", CONV3, "map", 99), "op 6 (conv_bn) layer 3: kernel map 99 missing or of another volume"),
    ("map of another volume", setter("ops", CONV3, "map", 5), "op 6 (conv_bn) layer 3: kernel map 5 missing or of another volume"),
    ("map that does not join", setter("maps", 1, "n_out", 601), "op 6 (conv_bn) layer 3: kernel map 1 is (600 -> 601), the slots hold (600 -> 600)"),
    ("direct route on a 3x3x3 layer", set_route(CONV3, ne.ROUTES["direct"]),
     "op 6 (conv_bn) layer 3: the direct route needs a transposed layer on a map whose pairs cover every output row once"),
    ("null neighbour table", lambda t: (set_route(CONV3, ne.ROUTES["ostat"])(t), setter("maps", 1, "nbr", 0)(t)), "op 6 (conv_bn): null neighbour table in map 1"),
    ("null position table", setter("maps", 1, "pos", 0), "op 6 (conv_bn): null position table in map 1"),
    ("a code that is no route", set_route(CONV3, 9), "op 6 (conv_bn) layer 3: route 9 is not one this entry point takes"),
    ("residual of another level", setter("ops", 7, "src2", 3), "op 7 (conv_bn): the residual slot does not match the output"),
    ("pv index out of range", setter("ops", VOX, "map", 7), "op 4 (voxelize): point-voxel index 7 out of range"),
    ("pv of the wrong level", setter("pvs", 0, "level", 2), "op 2 (devoxelize): point-voxel index 0 does not join these slots"),
    ("devoxelise changes the channel count", setter("ops", DEVOX, "channels", 64), "op 2 (devoxelize): channel counts differ"),
    ("null corner table", setter("pvs", 0, "devox_idx", 0), "op 2 (devoxelize): null corner table in index 0"),
    ("concat channels that do not add up", setter("ops", CONCAT, "channels", 388), "op 34 (concat): channel counts do not add up"),
    ("add of different levels", setter("ops", ADD, "level", 4), "op 30 (add): operands of different levels"),
    ("destination written twice", setter("ops", DEVOX, "dst", 2), "op 2 (devoxelize): slot 2 is written twice"),
    ("output slot on a voxel level", setter("ops", VOX, "dst", ne.SLOT_OUTPUT), "op 4 (voxelize): the output slot holds point rows"),
    ("ADD_EXT with dst != src", setter("ops", EXT, "dst", 3), "op 3 (add_ext): the fusion addend is added in place to an arena slot (layer = 0 early, 1 middle)"),
    ("slot read before it is written", setter("ops", STEM2, "src", 200), "op 1 (conv_bn): source slot 200 is not written before it is read"),
    ("huge map count", setter("maps", 4, "n_pairs", 1 << 31), "map 4 has a negative or huge count"),
]


@pytest.mark.parametrize("name,mutate,text", SHARED, ids=[c[0] for c in SHARED])
def test_shared_conditions_refuse_the_same_tables_with_the_same_text(ftx_lib, programs, name, mutate, text):
    ev, fwd, bwd = answers(ftx_lib, *both(programs, mutate))
    assert refused(ev, EVAL + text), ev
    assert refused(fwd, TRAIN + text) and refused(bwd, TRAIN + text), (fwd, bwd)


def test_null_tables_and_counts_are_refused_alike(ftx_lib, programs):
    ev, tr = both(programs)
    P = lambda a: None if a is None else ne._ptr(a)
    counts = [len(ev[0]), len(ev[1]), len(ev[3]), len(ev[4])]

    def texts(null=None, n=counts):
        e, t = ([None if j == null else a for j, a in enumerate(x)] for x in (ev, tr))
        assert ftx_lib.ftx_spvcnn_eval_arena_bytes(P(e[0]), n[0], P(e[1]), n[1], P(e[2]), P(e[3]), n[2], P(e[4]), n[3], P(e[5])) == 0
        a = ftx_lib.ftx_last_error().decode()
        assert ftx_lib.ftx_spvcnn_train_arena_bytes(P(t[0]), n[0], P(t[1]), n[1], P(t[2]), P(t[3]), n[2], P(t[4]), n[3], P(t[5]), P(t[6])) == 0
        return a, ftx_lib.ftx_last_error().decode()

    first, second = "null table or op count outside [1, 4096]", "null table"
    for null, text in ((1, first), (2, first), (5, first), (0, second), (3, second), (4, second)):
        assert texts(null) == (EVAL + text, TRAIN + text), null
    for i, n, text in ((1, 0, first), (1, 4097, first), (0, -1, second), (2, -1, second), (3, -1, second)):
        assert texts(n=counts[:i] + [n] + counts[i + 1:]) == (EVAL + text, TRAIN + text), (i, n)
    # the gradient routes are the training executor's: the eval entry has no such argument
    assert ftx_lib.ftx_spvcnn_train_arena_bytes(*[P(a) if not isinstance(a, int) else a for a in
                                                  (tr[0], counts[0], tr[1], counts[1], tr[2], tr[3], counts[2], tr[4], counts[3], tr[5], None)]) == 0
    assert ftx_lib.ftx_last_error().decode() == TRAIN + first
    # fewer maps or indices than the program uses
    assert texts(n=[counts[0], counts[1], 5, counts[3]]) == tuple(w + "op 5 (conv_bn) layer 2: kernel map 5 missing or of another volume" for w in (EVAL, TRAIN))
    assert texts(n=[counts[0], counts[1], counts[2], 1]) == tuple(w + "op 28 (devoxelize): point-voxel index 1 out of range" for w in (EVAL, TRAIN))


def last_op_dropped(t):
    for k in ("ops", "routes", "groutes"):
        if k in t:
            t[k] = t[k][:LAST]


def stem_residual_from_the_input(t):
    """One 1x1 layer on the input features with the input features as its residual: the smallest program with that operand."""
    t["layers"][0]["co"], t["layers"][0]["kvol"] = 4, 1
    op = t["ops"][0]
    op["map"], op["src2"], op["channels"] = -1, ne.SLOT_INPUT, 4
    t["routes"][0] = ne.ROUTE_ROWS
    for k in ("ops", "routes", "groutes"):
        if k in t:
            t[k] = t[k][:1]


def devoxelise_the_input(t):
    op = t["ops"][0]
    op["kind"], op["layer"], op["map"], op["level"], op["channels"] = ne.OP_DEVOXELIZE, -1, 0, ne.POINTS, 4
    for k in ("ops", "routes", "groutes"):
        if k in t:
            t[k] = t[k][:1]


def gap_in_the_segments(t):
    seg = t["ops"]["segment"]
    seg[seg >= 1] += 1


def addend_after_a_reader(t):
    """The middle addend lands on z0, which the voxelise and the first point transform have read by then."""
    op = t["ops"][EXT2]
    op["src"], op["dst"], op["channels"] = 4, 4, 32


# one mutation per condition that differs -> what the eval executor and the training executor answer (None: the tables are accepted)
DIFFER = [
    ("rows per level: an empty batch", dict(rows=[0] * 6, pairs=[0] * 5), None, None,
     "rows[0] = 0 (the training BatchNorm needs at least one row on every level)"),
    ("rows per level: one empty level", dict(rows=[5, 4, 3, 2, 0, 9], pairs=[5, 4, 3, 2, 0]), None, None,
     "rows[4] = 0 (the training BatchNorm needs at least one row on every level)"),
    ("rows per level: a negative count", {}, set_rows(3, -1), "rows[3] = -1 out of range",
     "rows[3] = -1 (the training BatchNorm needs at least one row on every level)"),
    ("rows per level: too many", {}, set_rows(2, 1 << 31), "rows[2] = 2147483648 out of range",
     "rows[2] = 2147483648 (the training BatchNorm needs at least one row on every level)"),
    ("segments: a gap", {}, gap_in_the_segments, "op 31 (add_ext): segments must be 0..2 and ascending",
     "op 3 (add_ext): segments are numbered from 0 without a gap, ascending, at most 8"),
    ("segments: descending", {}, setter("ops", CONV3, "segment", 0), "op 6 (conv_bn): segments must be 0..2 and ascending",
     "op 6 (conv_bn): segments are numbered from 0 without a gap, ascending, at most 8"),
    ("layer channels: more than 512 out of a sparse layer", {}, lambda t: (setter("layers", 3, "co", 516)(t), setter("ops", CONV3, "channels", 516)(t)),
     "op 7 (conv_bn) layer 4: channel counts do not match the slots", "op 6 (conv_bn) layer 3: channels must be multiples of 4 (ca=32 co=516)"),
    ("sparse layer: the pair list of the side the forward does not read", {}, setter("maps", 1, "pair_out", 0), None,
     "op 6 (conv_bn): null pair list in map 1 (the weight gradient reads both sides)"),
    ("sparse layer: the pair list of the side the forward reads", {}, setter("maps", 1, "pair_in", 0), "op 6 (conv_bn): null pair list in map 1",
     "op 6 (conv_bn): null pair list in map 1 (the weight gradient reads both sides)"),
    ("sparse layer: no offset table", {}, setter("maps", 1, "koff", 0), "op 6 (conv_bn): null pair list in map 1", "op 6 (conv_bn): null offset table in map 1"),
    ("sparse layer: a map without pairs and without tables", {}, no_pairs(1, null=("nbr", "pair_in", "pair_out", "koff")), None,
     "op 6 (conv_bn): null offset table in map 1"),
    ("output-stationary route on a map without pairs", {}, no_pairs(1, CONV3, ne.ROUTES["ostat"]), None,
     "op 6 (conv_bn) layer 3: the output-stationary route does not take this layer"),
    ("pairs route on a map without pairs", {}, no_pairs(1), None, "op 6 (conv_bn) layer 3: the empty route is for a map without pairs, and only for it"),
    ("empty route on a map with pairs", {}, set_route(CONV3, ne.ROUTES["empty"]), "op 6 (conv_bn) layer 3: the empty route on a map with pairs",
     "op 6 (conv_bn) layer 3: the empty route is for a map without pairs, and only for it"),
    ("residual slot: the input features", {}, stem_residual_from_the_input, None, "op 0 (conv_bn): the residual slot does not match the output"),
    ("devoxelise: the input features", {}, devoxelise_the_input, None, "op 0 (devoxelize): channel counts differ"),
    ("voxelise: no unsorted index", {}, setter("pvs", 1, "vox_idx", 0), None, "op 32 (voxelize): null voxel index in index 1 (the backward reads it)"),
    ("voxelise: no sorted segments", {}, setter("pvs", 1, "vox_seg_off", 0), "op 32 (voxelize): null sorted segments in index 1", None),
    ("add: one slot twice", {}, setter("ops", ADD, "src2", 29), None, "op 30 (add): operands of different levels"),
    ("ADD_EXT: after a reader of its slot", {}, addend_after_a_reader, None,
     "op 31 (add_ext): slot 4 is read before the addend reaches it, and the backward would read it after"),
    ("destination: a layer writes the output slot", {}, setter("ops", LAST_LINEAR, "dst", ne.SLOT_OUTPUT), "op 67 (add): operands of different levels",
     "op 66 (linear_bn): a layer may not write the output slot (its backward reads its result, which the backward is not given)"),
    ("after the loop: the output slot is never written", {}, last_op_dropped, None, "the last op writes the output slot"),
    ("a third gradient contribution", {}, setter("ops", 65, "src", 62), None,
     "op 65 (devoxelize): slot 62 would receive more than two gradient contributions"),
]


@pytest.mark.parametrize("name,kw,mutate,eval_text,train_text", DIFFER, ids=[c[0] for c in DIFFER])
def test_the_executors_diverge_exactly_where_listed(ftx_lib, programs, name, kw, mutate, eval_text, train_text):
    ev, fwd, bwd = answers(ftx_lib, *both(programs, mutate, **kw))
    assert accepted(ev) if eval_text is None else refused(ev, EVAL + eval_text), ev
    for a in (fwd, bwd):
        assert accepted(a) if train_text is None else refused(a, TRAIN + train_text), a


def test_gradient_routes_are_the_training_executors_alone(ftx_lib, programs):
    program, tp = programs
    for op, route, text in ((CONV3, ne.ROUTES["direct"], "op 6 (conv_bn) layer 3: the direct gradient route needs a strided layer on a map whose pairs cover every input row once"),
                            (CONV3, ne.ROUTES["empty"], "op 6 (conv_bn) layer 3: the empty gradient route on a map with pairs"),
                            (DOWN, ne.ROUTES["pairs"], None), (DOWN, ne.ROUTES["ostat"], "op 5 (conv_bn) layer 2: gradient route 2 is not one this entry point takes"),
                            (0, 9, None)):      # the first convolution reads the input features: its gradient route is not looked at
        tr = list(th.train_tables(tp))
        tr[6][op] = route
        _, fwd, bwd = answers(ftx_lib, eh.tables(program), tuple(tr))
        for a in (fwd, bwd):
            assert accepted(a) if text is None else refused(a, TRAIN + text), a
    # the position table of the input side: the forward does not read it, the pair-list gradient does
    ev, fwd, bwd = answers(ftx_lib, *both(programs, setter("maps", 1, "pos_t", 0)))
    text = TRAIN + "op 6 (conv_bn) layer 3: the pair-list gradient route needs pairs and the position table of the input side"
    assert accepted(ev) and refused(fwd, text) and refused(bwd, text)


def test_arena_sizes_of_the_standard_tables(ftx_lib, programs):
    """Placement is each executor's own and consumes what the checker found: the sizes are those of the two separate checkers."""
    full = dict(rows=[81237, 43016, 20197, 8102, 2949, 81237], pairs=[382735, 219664, 126675, 56976, 20329])
    sizes = [[eh.size(ftx_lib, ev), th.size(ftx_lib, tr)] for ev, tr in (both(programs), both(programs, **full), both(programs, rows=[1] * 6, pairs=[1] * 5))]
    assert sizes == [[9666560, 50567936], [629864448, 2816493312], [15616, 11175168]], sizes
    assert eh.size(ftx_lib, both(programs, rows=[0] * 6, pairs=[0] * 5)[0]) == 256
