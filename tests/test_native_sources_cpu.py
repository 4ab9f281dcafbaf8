"""Every file libmdpt.so is compiled from is a dependency native._stale() watches and native.source_hash() hashes: the #include "..." lines are walked
transitively from every source, and each must resolve to a file of native.SOURCES + native.HEADERS. (A header left out is edited without a rebuild
and without a new stamp on the measurements taken with it.)"""
import os
import re

from muggled_dpt_amd import native

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
SEARCH = (native.CSRC, os.path.join(native.REPO, "include"))  # the -I directories of native.build()


def _covered():
    return [os.path.join(native.CSRC, s) for s in native.SOURCES] + [h if os.path.isabs(h) else os.path.join(native.CSRC, h) for h in native.HEADERS]


def test_every_quoted_include_is_a_tracked_dependency():
    covered = {os.path.realpath(p) for p in _covered()}
    todo, seen = [os.path.join(native.CSRC, s) for s in native.SOURCES], set()
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        with open(path) as fh:
            for name in INCLUDE.findall(fh.read()):
                found = [os.path.join(d, name) for d in (os.path.dirname(path), *SEARCH) if os.path.isfile(os.path.join(d, name))]
                assert found, f"{os.path.relpath(path, native.REPO)} includes {name}, which is in none of the include directories"
                assert os.path.realpath(found[0]) in covered, f"{name} (included by {os.path.relpath(path, native.REPO)}) is not in native.HEADERS"
                todo.append(found[0])
    # what started this test: the fp8 cross terms, the dtype loads, and the files postprocess.hip and elementwise.hip are made of
    names = {os.path.basename(p) for p in seen}
    assert {"f8_cross.h", "dt_io.h", "post_common.inc", "ew_common.inc", "mdpt.h"} <= names


def test_no_dependency_is_listed_twice_and_the_order_is_fixed():
    paths = [os.path.realpath(p) for p in _covered()]
    assert len(paths) == len(set(paths)) and all(os.path.isfile(p) for p in paths)
    in_csrc = [h for h in native.HEADERS if not os.path.isabs(h)]
    assert in_csrc == sorted(in_csrc)  # (source_hash() covers the names: it must not depend on the directory's listing order)
