"""CPU: what the sort-free PPMI assembly of a store batch (csrc/gda_collate.hip ``gda_collate_ppmi_csr_f32``) promises
before anything touches a device -- its argument checks, an empty batch that launches nothing -- that the header, the
``_lib`` table and INTEGRATION.md name the same symbol, and that a trainer over CPU stores still runs today's eager
loop with today's numbers.  What the entry point computes is tested in tests/test_gpu_collate_ppmi_csr.py."""
import ctypes
import os
import re

import torch

from pygda_amd import _lib
from pygda_amd.data import GraphStore
from tests.test_graph_store_host import _dataset, _run
from tests.conftest import load_golden

NULL, SIZE, ALIAS = -1, -2, -5
SYMBOL = "gda_collate_ppmi_csr_f32"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def P(addr):
    return ctypes.c_void_p(addr)


# distinct non-NULL dummies: validation comes first, nothing is dereferenced
IDS, NPTR, SEG, BATCH, EOFF, PPTR, POFF, W, DIS = (P(0x1000 * k) for k in range(1, 10))
STRUCT = tuple(P(0x100000 + 0x1000 * k) for k in range(6))       # rowptr, colidx, pair_of, t_rowptr, t_colidx, t_pair_of
OUTS = tuple(P(0x200000 + 0x1000 * k) for k in range(6))         # rowptr, colidx, val, t_rowptr, t_colidx, t_val


def ppmi_csr(ids=IDS, B=4, G=9, node_ptr=NPTR, seg=SEG, batch=BATCH, n=20, eoff=EOFF, nnz=60, struct=STRUCT, total=500,
             pair_ptr=PPTR, pair_off=POFF, w=W, m=45, fill=1.0, outs=OUTS, dis=DIS):
    return getattr(_lib.lib(), SYMBOL)(ids, B, G, node_ptr, seg, batch, n, eoff, nnz, *struct, total, pair_ptr, pair_off, w,
                                       m, fill, *outs, dis, None)


def _swap(seq, k, v):
    return tuple(v if i == k else a for i, a in enumerate(seq))


def test_the_ppmi_assembly_validates_its_arguments():
    for missing in ("ids", "node_ptr", "seg", "batch", "eoff", "pair_ptr", "pair_off", "w", "dis"):
        assert ppmi_csr(**{missing: None}) == NULL, missing
    for k in range(6):
        assert ppmi_csr(struct=_swap(STRUCT, k, None)) == NULL and ppmi_csr(outs=_swap(OUTS, k, None)) == NULL, k
    for bad in (dict(B=-1), dict(G=-1), dict(n=-1), dict(nnz=-1), dict(total=-1), dict(m=-1),
                dict(n=2 ** 31 - 1, nnz=2 ** 31 - 1), dict(nnz=2 ** 31)):
        assert ppmi_csr(**bad) == SIZE, bad
    # zero capacity: every row holds at least its loop, and entries come out of a store that has some
    assert ppmi_csr(nnz=0) == SIZE and ppmi_csr(nnz=19) == SIZE and ppmi_csr(total=0) == SIZE
    for k in (0, 1, 3, 4):                                         # an output on top of the structure it is gathered from
        assert ppmi_csr(outs=_swap(OUTS, k, STRUCT[k])) == ALIAS, k
    for k in range(6):
        assert ppmi_csr(outs=_swap(OUTS, k, OUTS[(k + 3) % 6])) == ALIAS, k
    assert ppmi_csr(dis=OUTS[2]) == ALIAS and ppmi_csr(dis=OUTS[5]) == ALIAS
    assert ppmi_csr(w=OUTS[2]) == ALIAS and ppmi_csr(w=OUTS[5]) == ALIAS and ppmi_csr(w=DIS) == ALIAS
    # no room for a row: the row and entry operands may be missing, the rest may not
    assert ppmi_csr(n=0, nnz=0, batch=None, dis=None, struct=_swap(_swap(STRUCT, 1, None), 2, None), ids=None) == NULL


def test_an_empty_batch_launches_nothing_and_looks_at_no_operand():
    none6 = (None,) * 6
    assert ppmi_csr(B=0, ids=None, node_ptr=None, seg=None, batch=None, eoff=None, pair_ptr=None, pair_off=None, w=None, dis=None,
                    struct=none6, outs=none6, n=0, nnz=0, total=0, m=0) == 0


def test_header_table_and_integration_guide_name_the_same_symbol():
    header = open(os.path.join(ROOT, "include", "gda_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(rf"\bint {SYMBOL}\s*\(", code)
    assert SYMBOL in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), SYMBOL)
    assert f"`{SYMBOL}`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # one argument per parameter of the declaration
    decl = re.search(rf"\bint {SYMBOL}\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_lib._SIGNATURES[SYMBOL][1])


def test_a_cpu_store_trainer_still_trains_eagerly_with_the_same_numbers():
    g = load_golden("a2gnn_graph_fit3_b6")
    src, tgt = _dataset(g, "src"), _dataset(g, "tgt")
    for batch_size in (0, 6):
        want = _run("grade", batch_size, src, tgt)
        got = _run("grade", batch_size, GraphStore(src, "cpu"), GraphStore(tgt, "cpu"))
        assert got[0] == want[0] and len(got[0]) == 3
        assert all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
        assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]) and torch.equal(got[4], want[4])
