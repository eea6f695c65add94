"""A stand-in for the ``ops`` / ``gemm_plan`` modules of models/llama.py that logs the kernel calls a forward
path makes, on the CPU (tests/test_step_plan.py, tests/test_layer_paths.py)."""


class Recorder:
    """Logs every call as ``(name, kwargs)`` and returns ``ret`` — or, when ``ret`` is callable,
    ``ret(name, args, kwargs)``.  The calls that return two values return the pair ``(ret, ret)``; the host-side
    predicates are answered here and not logged (they launch nothing)."""
    Fp8Weight = type("Fp8Weight", (), {})
    MXAct = type("MXAct", (), {})
    PAIRS = ("linear_fp8_swiglu", "linear_fp8_swiglu_mx")

    def __init__(self, log, ret):
        self._log, self._ret = log, ret

    def split_plan(self, *a):
        return (2, 0)

    def dense_mx_ok(self, *a):
        return False

    def __getattr__(self, name):
        def call(*a, **kw):
            self._log.append((name, kw))
            r = self._ret(name, a, kw) if callable(self._ret) else self._ret
            return (r, r) if name in self.PAIRS else r
        return call
