"""The six entries that take a table of column pointers (mbls_fr_eval_program, mbls_fr_eval_graph,
mbls_fr_lookup_multiplicities, mbls_fr_logup_sum, mbls_fr_inner_products, mbls_fr_multi_eval), each run
with every operand on the host and with every operand on the device: the two results are equal word
for word, and at 9 rows equal to the entry's Python model.  A host table is staged by the library, one
member per aligned stride; a device table is read where it lies.  At 9 rows a column is 288 bytes and
its stride 512, so members packed by bytes where the stride is meant, or the reverse, read the wrong
rows; 1 row is the degenerate table; 257 rows cross the expression kernel's 256-row tile with a staged
column.  The logup entries take 1 input and the most, 64."""
import functools
import random

import numpy as np
import pytest

import expr_model as E
import graph_model as G
import inner_model as IM
import logup_model as LM

pytestmark = pytest.mark.gpu

R = E.R
ROWS = (1, 9, 257)
MODEL_ROWS = 9
MOST_INPUTS = 64


def _amd():
    """the binding, with torch imported before the library is loaded"""
    import torch  # noqa: F401
    import gpu_helpers
    return gpu_helpers.amd


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _amd().lib()
    return _amd()


def words(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def ints(arr):
    data = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


def dev(a):
    return _amd().torch_u64(np.ascontiguousarray(a))


def on_host(a):
    return a


def host(x):
    """a result as host words, whichever side it was placed on"""
    return x if isinstance(x, np.ndarray) else _amd().to_numpy_u64(x)


@functools.lru_cache(maxsize=None)
def bank():
    """MOST_INPUTS columns of max(ROWS) stored values, no two alike: mostly from a pool of 61 values
    (so the inputs of a lookup meet its table), with 0, 1 and r - 1 among them"""
    rnd = random.Random(2718)
    pool = [0, 1, R - 1] + [rnd.randrange(R) for _ in range(58)]
    return [[rnd.choice(pool) for _ in range(max(ROWS))] for _ in range(MOST_INPUTS)]


def columns(k, n, first=0):
    return [c[:n] for c in bank()[first:first + k]]


CONSTS = [random.Random(3141).randrange(R) for _ in range(2)]
BETA, INIT = (random.Random(1618).randrange(1, R) for _ in range(2))

# every column of a table of 1 and of 3 is read, the last one at a rotated row
EXPR = {1: [(E.COLUMN, 0, 1), (E.COLUMN, 0, 0), (E.MUL, 0, 0), (E.CONST, 1, 0), (E.ADD, 0, 0), (E.EMIT, 0, 0)],
        3: [(E.COLUMN, 0, 1), (E.COLUMN, 1, 0), (E.MUL, 0, 0), (E.COLUMN, 2, -1), (E.HORNER, 0, 0), (E.EMIT, 0, 0),
            (E.COLUMN, 2, 0), (E.EMIT, 1, 0)]}
_V, _C, _K, _NO = G.val, G.col, G.const, G.NO
GRAPH = {1: [(G.MUL, _C(0, 1), _C(0), 0), (G.ADD, _V(0), _K(1), 0), (G.EMIT, _V(1), _NO, 0)],
         3: [(G.MUL, _C(0, 1), _C(1), 0), (G.HORNER, _V(0), _C(2, -1), 0), (G.MUL, _V(1), _V(0), 0),
             (G.EMIT, _V(2), _NO, 0), (G.STORE, _C(2), _NO, 0), (G.EMIT, _V(4), _NO, 1)]}


def evaluator(amd, which, k, n, place):
    run = amd.eval_program if which == "expr" else amd.eval_graph
    prog = (EXPR if which == "expr" else GRAPH)[k]
    return [run([place(words(c)) for c in columns(k, n)], prog, constants=place(words(CONSTS)), n_outputs=(k + 1) // 2)]


def evaluator_model(which, k, n):
    run, prog = (E.run, EXPR[k]) if which == "expr" else (G.run, GRAPH[k])
    return [sum(run(columns(k, n), prog, CONSTS, (k + 1) // 2), [])]


def table_and_m(n):
    table = bank()[MOST_INPUTS - 1][:n]
    return table, bank()[MOST_INPUTS - 2][:n]  # any m, not only the right one


def multiplicities(amd, k, n, place):
    table, _ = table_and_m(n)
    m, missing = amd.lookup_multiplicities([place(words(c)) for c in columns(k, n)], place(words(table)))
    return [m, np.array(missing, dtype=np.uint64)]


def multiplicities_model(k, n):
    counts, missing = LM.multiplicities_ref(columns(k, n), table_and_m(n)[0])
    return [LM.count_elements(counts), [missing]]


def logup_sum(amd, k, n, place):
    table, m = table_and_m(n)
    out, total = (None, True) if place is on_host else (amd.torch_u64((n, 4)), amd.torch_u64((1, 4)))
    return list(amd.logup_sum([place(words(c)) for c in columns(k, n)], place(words(table)), place(words(m)),
                              place(words([BETA])), place(words([INIT])), out=out, total=total))


def logup_sum_model(k, n):
    table, m = table_and_m(n)
    out, total = LM.logup_sum_ref(columns(k, n), table, m, BETA, INIT)
    return [out, [total]]


def inner_products(amd, n, place_columns, place_vectors):
    return [amd.inner_products([place_columns(words(c)) for c in columns(3, n)],
                               [place_vectors(words(c)) for c in columns(2, n, first=3)])]


def multi_eval(amd, n, place):
    return [amd.multi_eval([place(words(c)) for c in columns(3, n)], place(words(CONSTS)))]


def agree(results, model, what):
    """every result of `results` (one list of arrays per placement) is the first, word for word, and
    the model's integers when there is a model"""
    first = [host(x) for x in results[0]]
    for other in results[1:]:
        assert len(other) == len(first), what
        for a, b in zip(first, other):
            assert np.array_equal(a, host(b)), what
    if model is not None:
        assert [ints(a) if a.ndim == 2 else a.tolist() for a in first] == model, what


@pytest.mark.parametrize("n", ROWS)
def test_host_and_device_tables_agree(amd, n):
    with_model = n == MODEL_ROWS
    for which in ("expr", "graph"):
        for k in (1, 3):
            agree([evaluator(amd, which, k, n, p) for p in (on_host, dev)],
                  evaluator_model(which, k, n) if with_model else None, (which, k))
    for k in (1, MOST_INPUTS):
        agree([multiplicities(amd, k, n, p) for p in (on_host, dev)], multiplicities_model(k, n) if with_model else None,
              ("multiplicities", k))
        agree([logup_sum(amd, k, n, p) for p in (on_host, dev)], logup_sum_model(k, n) if with_model else None,
              ("logup_sum", k))
    # the two tables of one call placed alike, and oppositely
    agree([inner_products(amd, n, pc, pv) for pc, pv in ((on_host, on_host), (dev, dev), (on_host, dev), (dev, on_host))],
          [IM.inner_products_ref(columns(3, n), columns(2, n, first=3))] if with_model else None, "inner_products")
    agree([multi_eval(amd, n, p) for p in (on_host, dev)],
          [IM.multi_eval_ref(columns(3, n), CONSTS)] if with_model else None, "multi_eval")
