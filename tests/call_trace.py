"""Shared by the call-trace tests (tests/test_pipeline_call_trace.py, tests/test_batch_call_trace.py): the recorder _lib.load() hands out
while a scenario runs, and what a trace holds of a pipeline afterwards.  Each test passes its own table of plain integer arguments."""
import contextlib

# when a pipeline or a stream is let go of is the garbage collector's business, not a pass's
UNORDERED = ("urhgpu_ctx_destroy", "urhgpu_stream_destroy")


class Recorder:
    """forwards to the loaded library and notes the name of every urhgpu_* function called, with its plain integer arguments:
    int_args is {name: positions} -- flags, lengths, capacities; never an address or a size made from one"""

    def __init__(self, lib, int_args):
        self.__dict__.update(_lib=lib, _int_args=int_args, log=[])

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("urhgpu_") or name in UNORDERED:
            return fn

        def call(*args):
            plain = [args[i].decode() if isinstance(args[i], bytes) else int(args[i]) for i in self._int_args.get(name, ())]
            self.log.append(" ".join([name] + [str(v) for v in plain]))
            return fn(*args)
        return call


@contextlib.contextmanager
def recording(int_args):
    """_lib.load() hands out the recorder: every call of the package into the library, Context's methods included, goes through it"""
    from urh_amd import _lib
    _lib.host_libm_verdict()                                   # (once per process, whoever comes first: not a pass's call)
    real = _lib.load
    rec = Recorder(real(), int_args)
    _lib.load = lambda: rec
    try:
        yield rec
    finally:
        _lib.load = real


def sizes(d):
    return {str(k): int(v.numel()) for k, v in d.items() if hasattr(v, "numel")}


def trace(rec, pipe, results):
    return {"calls": list(rec.log), "bufs": sizes(pipe._bufs), "pinned": sizes(pipe._pinned), "results": results}
