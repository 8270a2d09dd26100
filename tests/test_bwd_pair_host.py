"""CPU: argument validation of the entry point that runs a layer's data gradient and weight gradient in one launch
(gda_gemm_act_cm_bwd_f32).  Status codes come back before anything touches a device."""
import ctypes

from pygda_amd import _lib

NULL, SIZE, WORKSPACE, UNSUPPORTED, ALIAS = -1, -2, -3, -4, -5


def P(addr):
    return ctypes.c_void_p(addr)


# distinct non-NULL dummies, 16-byte aligned: validation comes first, nothing is dereferenced
GT, W, Y, GXT, GW, WS = (P(0x1000 * k) for k in range(1, 7))


def cm_bwd(n=8, M=128, K=128, gT=GT, ldT=8, w=W, ldw=None, y=Y, p=0.5, gxT=GXT, gW=GW, ws=None, ws_bytes=0):
    return _lib.lib().gda_gemm_act_cm_bwd_f32(n, M, K, gT, ldT, w, K if ldw is None else ldw, y, p, gxT, gW, ws, ws_bytes, None)


def test_gemm_act_cm_bwd_validates_its_arguments():
    for missing in ("gT", "w", "y"):
        assert cm_bwd(**{missing: None}) == NULL, missing
    assert cm_bwd(n=9, ldT=8) == SIZE                       # ldT < n
    assert cm_bwd(ldw=64) == SIZE                           # ldw < K
    assert cm_bwd(n=-1) == SIZE and cm_bwd(M=-1) == SIZE and cm_bwd(K=-4) == SIZE
    assert cm_bwd(p=1.0) == SIZE and cm_bwd(p=-0.1) == SIZE
    for out in ("gxT", "gW"):
        for other in (GT, W, Y):
            assert cm_bwd(**{out: other}) == ALIAS, out
    assert cm_bwd(gW=GXT) == ALIAS
    assert cm_bwd(K=130) == UNSUPPORTED                     # K % 4
    assert cm_bwd(M=6) == UNSUPPORTED                       # M % 4
    assert cm_bwd(ldw=130) == UNSUPPORTED                   # rows of W not 16-byte aligned
    assert cm_bwd(w=P(0x2004)) == UNSUPPORTED and cm_bwd(y=P(0x3008)) == UNSUPPORTED
    assert cm_bwd(M=132) == UNSUPPORTED and cm_bwd(M=256) == UNSUPPORTED    # the composition's dgrad is split there
    assert cm_bwd(n=0, ldT=0) == UNSUPPORTED and cm_bwd(M=0) == UNSUPPORTED      # zero fills: left to the caller
    # from 1024 nodes on the weight gradient is split over row slabs: its partials need the workspace of the NN product
    L = _lib.lib()
    need = L.gda_gemm_workspace_bytes(1, 128, 128, 2048)
    assert need == 16 * 128 * 129 * 4
    assert cm_bwd(n=2048, ldT=2048) == WORKSPACE
    assert cm_bwd(n=2048, ldT=2048, ws=WS, ws_bytes=need - 1) == WORKSPACE


def test_gemm_act_cm_bwd_with_nothing_to_do_looks_at_no_operand():
    assert cm_bwd(gxT=None, gW=None, gT=None, w=None, y=None) == 0               # neither output wanted
    assert cm_bwd(K=0, gT=None, w=None, y=None, gxT=None, gW=None) == 0
    assert cm_bwd(K=0, gT=None, w=None, y=None) == 0                             # both outputs empty


def test_the_flag_is_a_module_constant():
    from pygda_amd import ops
    assert ops.BWD_PAIR is True
