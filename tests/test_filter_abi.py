"""The ABI of facet filters on phrase and group queries (fg_filter_clauses,
DESIGN.md §16): ONE new symbol -- FG_ABI_VERSION stays 6 and fg_query_batch keeps
its layout.  Without a device: the header, the Rust binding, the Python binding
and the library agree, and the switch keeps the contract of its twins."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture()
def switch():
    """sets fg_filter_clauses; the setting found is restored in teardown"""
    from fugu_amd import native
    was = native.filter_clauses()
    yield native.filter_clauses
    native.filter_clauses(was)


def test_header_rust_python_and_library_agree():
    from fugu_amd import native
    h = open(os.path.join(ROOT, "include", "fugu.h")).read()
    rs = open(os.path.join(ROOT, "rust", "ffi.rs")).read()
    assert re.search(r"\nint fg_filter_clauses\(int on\);", h)
    assert "pub fn fg_filter_clauses(on: c_int) -> c_int;" in rs
    assert re.search(r"#define FG_ABI_VERSION 6\b", h) and native.ABI_VERSION == 6
    assert native.lib().fg_abi_version() == 6
    assert [n for n, _ in native.QueryBatch._fields_] == ["n_queries", "q_off", "terms", "mode", "f_off", "f_terms",
                                                          "occur", "phrase_len", "phrase_pos"]
    assert "fg_filter_clauses" in native.EXPORTS
    lib = ctypes.CDLL(native.LIB_PATH)  # the symbol itself, not the binding's wrapper
    assert lib.fg_filter_clauses is not None and hasattr(native.lib(), "fg_filter_clauses")
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "fg_filter_clauses" in open(os.path.join(ROOT, doc)).read(), doc


def test_switch_contract(switch):
    from fugu_amd import native
    assert switch() == 0  # off by default
    assert switch(1) == 0 and switch(-1) == 1 and switch(-7) == 1  # returns the previous setting; < 0 only asks
    assert (native.phrase_clauses(), native.group_clauses()) == (0, 0)  # its twins are switches of their own
    assert switch(5) == 1 and switch(0) == 1 and switch() == 0
    was = native.group_clauses(1)
    try:
        assert switch() == 0
    finally:
        native.group_clauses(was)


def test_null_arguments_still_fail_cleanly(switch):
    from fugu_amd import native
    switch(1)
    assert native.lib().fg_plan_create(None, None, 10, None) == native.FG_EINVAL
