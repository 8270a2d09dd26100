"""CPU: argument validation of the two projections that apply the upstream activation on their operand load
(gda_gemm_act_cm_f32, gda_gemm_skinny_act_cm_f32).  Status codes come back before anything touches a device."""
import ctypes

from pygda_amd import _lib

NULL, SIZE, UNSUPPORTED, ALIAS = -1, -2, -4, -5


def P(addr):
    return ctypes.c_void_p(addr)


# distinct non-NULL dummies, 16-byte aligned: validation comes first, nothing is dereferenced
XT, W, Y, HT, STEP = P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0x5000)


def act_cm(n=8, M=128, K=128, xT=XT, ldT=8, w=W, ldw=None, y=Y, hT=HT, ldc=8, p=0.5, step=STEP):
    return _lib.lib().gda_gemm_act_cm_f32(n, M, K, xT, ldT, w, K if ldw is None else ldw, y, hT, ldc, p, 1, step, 1, None)


def skinny(n=8, N=5, K=128, xT=XT, ldT=8, w=W, ldw=None, out=Y, ldy=None, p=0.5, step=STEP):
    return _lib.lib().gda_gemm_skinny_act_cm_f32(n, N, K, xT, ldT, w, K if ldw is None else ldw, out,
                                                 N if ldy is None else ldy, p, 1, step, 1, None)


def test_gemm_act_cm_validates_its_arguments():
    for missing in ("xT", "w", "hT", "step"):
        assert act_cm(**{missing: None}) == NULL, missing
    assert act_cm(n=9, ldT=8, ldc=12) == SIZE               # ldT < n
    assert act_cm(n=9, ldT=12, ldc=8) == SIZE               # ldc < n
    assert act_cm(ldw=64) == SIZE                           # ldw < K
    assert act_cm(n=-1) == SIZE
    assert act_cm(p=1.0) == SIZE and act_cm(p=-0.1) == SIZE
    assert act_cm(hT=XT) == ALIAS and act_cm(hT=W) == ALIAS
    assert act_cm(y=XT) == ALIAS and act_cm(y=W) == ALIAS and act_cm(y=HT) == ALIAS
    assert act_cm(K=130) == UNSUPPORTED                     # K % 4
    assert act_cm(K=0) == UNSUPPORTED
    assert act_cm(M=6) == UNSUPPORTED                       # M % 4
    assert act_cm(ldw=130) == UNSUPPORTED                   # rows of W not 16-byte aligned
    assert act_cm(w=P(0x2004)) == UNSUPPORTED and act_cm(y=P(0x3008)) == UNSUPPORTED
    # nothing to do: no operand is looked at
    assert act_cm(n=0, xT=None, w=None, y=None, hT=None, step=None) == 0
    assert act_cm(M=0, xT=None, w=None, y=None, hT=None, step=None) == 0


def test_gemm_skinny_act_cm_validates_its_arguments():
    for missing in ("xT", "w", "out", "step"):
        assert skinny(**{missing: None}) == NULL, missing
    assert skinny(n=9, ldT=8) == SIZE                       # ldT < n
    assert skinny(ldy=4) == SIZE                            # ldy < N
    assert skinny(ldw=64) == SIZE                           # ldw < K
    assert skinny(n=-1) == SIZE and skinny(p=1.0) == SIZE
    assert skinny(out=XT) == ALIAS and skinny(out=W) == ALIAS
    assert skinny(N=9) == UNSUPPORTED                       # more than 8 classes
    assert skinny(K=100) == UNSUPPORTED and skinny(K=512) == UNSUPPORTED
    assert skinny(n=0, xT=None, w=None, out=None, step=None) == 0
    assert skinny(N=0, xT=None, w=None, out=None, step=None) == 0


def test_the_flag_is_a_module_constant():
    from pygda_amd import ops
    assert ops.ACT_IN_CONSUMER is True
