"""The C ABI added for the Softplus / Sigmoid losses and Adagrad: exported symbols and the argument
checks that run before anything touches a device."""
import ctypes

import torch  # noqa: F401  (the library binds to torch's HIP runtime)

NEW = ("mmre_adagrad_step", "mmre_ns_forward_ex", "mmre_ns_backward_ex", "mmre_ns_fused_forward_ex",
       "mmre_ns_fused_grad_ex", "mmre_ns_fused_grad_sgd_ex", "mmre_ns_step_openke_gen_pipe_ex")


def test_new_symbols_exported():
    from mmre import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
    # the entry points without the suffix are still there (wrappers around their twins)
    for n in NEW[1:]:
        assert hasattr(L, n[:-3]), n[:-3]


def test_unknown_loss_kind_is_a_bad_argument():
    """Checked first, before any pointer is looked at: the (never dereferenced) addresses below are
    not device memory."""
    from mmre import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)
    for kind, opt, want in ((7, 0, 1), (-1, 0, 1), (1, 5, 1)):
        o = _lib.NSOpts(loss_kind=kind, optimizer=opt)
        rc = lib.mmre_ns_forward_ex(2, 0, 0.0, 0, fake, None, fake, None, 8, 0.0, fake, fake, fake, 4, 2, 0.0, 0.0, 0.0,
                                    fake, fake, fake, None, ctypes.byref(o))
        assert rc == want, (kind, opt, rc)
        rc = lib.mmre_ns_fused_grad_sgd_ex(2, 0, 0.0, 0, fake, None, fake, None, 10, 3, 8, 0.0, fake, fake, fake, 4, 2,
                                           0.0, 0.0, 0.0, fake, None, fake, None, fake, None, fake, 0.5, None,
                                           ctypes.byref(o))
        assert rc == want, (kind, opt, rc)
    assert _lib.LOSS_KINDS == {"margin": 0, "softplus": 1, "sigmoid": 2}


def test_adagrad_step_rejects_bad_arguments_without_a_device():
    from mmre import _lib
    lib = _lib.lib()
    arr = lambda vals: ctypes.cast((ctypes.c_void_p * len(vals))(*vals), ctypes.c_void_p)
    num = lambda vals: ctypes.cast((ctypes.c_int64 * len(vals))(*vals), ctypes.c_void_p)
    ok = [4096 + 64 * i for i in range(9)]
    # count outside 1..8
    assert lib.mmre_adagrad_step(arr(ok), arr(ok), arr(ok), num([4] * 9), 9, 0.5, 1e-10, None) == 1
    assert lib.mmre_adagrad_step(arr(ok), arr(ok), arr(ok), num([4] * 9), 0, 0.5, 1e-10, None) == 1
    # a parameter, gradient or sum that is not 16-B aligned
    for which in range(3):
        ptrs = [list(ok[:2]) for _ in range(3)]
        ptrs[which][1] += 4
        assert lib.mmre_adagrad_step(arr(ptrs[0]), arr(ptrs[1]), arr(ptrs[2]), num([4, 4]), 2, 0.5, 1e-10, None) == 1
    # null lists / entries, negative sizes
    assert lib.mmre_adagrad_step(None, arr(ok), arr(ok), num([4]), 1, 0.5, 1e-10, None) == 1
    assert lib.mmre_adagrad_step(arr([0]), arr(ok), arr(ok), num([4]), 1, 0.5, 1e-10, None) == 1
    assert lib.mmre_adagrad_step(arr(ok), arr(ok), arr(ok), num([-1]), 1, 0.5, 1e-10, None) == 1
    # nothing to do: no launch
    assert lib.mmre_adagrad_step(arr(ok), arr(ok), arr(ok), num([0, 0]), 2, 0.5, 1e-10, None) == 0
