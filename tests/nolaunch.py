"""A stand-in for libftx under which nothing can be launched: the safety net of every bad-operand test.

    monkeypatch.setattr(_lib, "load", lambda: NoLaunch())

Every `ftx_*` entry raises AssertionError("launched") when it is called, so an operand check that is missing fails the test at the
stub and never hands a short buffer to a kernel.  The host-only queries (workspace sizes, block counts, supported / tile questions,
the last error text) launch nothing and answer through the real library: functional.py caches some of their answers per shape, and a
made-up figure would outlive the test."""
from fusiontransformer_amd import _lib

_REAL_LOAD = _lib.load
HOST_ONLY_SUFFIXES = ("_workspace_bytes", "_arena_bytes", "_blocks", "_block_cols", "_supported", "_tile", "_bytes", "_capacity", "_ksize",
                      "_chunk_elements", "_layout_words")
HOST_ONLY = ("ftx_version", "ftx_last_error")


def _launched(*args):
    raise AssertionError("launched")


class NoLaunch:
    """Stands in for libftx: any launch is a test failure, so a bad operand can never reach a kernel."""

    def __getattr__(self, name):
        if not name.startswith("ftx_"):
            raise AttributeError(name)
        if name in HOST_ONLY or name.endswith(HOST_ONLY_SUFFIXES):
            return getattr(_REAL_LOAD(), name)
        return _launched
