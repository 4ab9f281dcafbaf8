#!/usr/bin/env python3
"""The refusals of the mdpt_post_* entry points as they are AT A COMMIT, written to tests/golden/post_refusals.json.

Runs the table of tests/post_refusal_cases.py against the built library and records, per case, the return code and the whole mdpt_last_error() text;
per accepted *_scratch_bytes query, the byte count. The header names the commit the library was built from: run this at the commit whose behaviour is
to be kept (with its csrc/ and include/ unchanged and its library built), not on the code that has to keep it.

It refuses to write a case that does not return MDPT_E_INVALID (a 0 or a HIP error reached a launch: a mistake in the table), and it reads the
post-processing host sources of that commit (csrc/mdpt_post*.cpp, mdpt_post_checks.h) to print "site (line) -> cases": every fail( site of the record
entry points (guided, refocus, normals, shadows), of every check_* helper and of the "scratch of %zu bytes" refusals must have a case, and every entry
point at least one. A case is matched to a site by its entry point (the site lies in it or in a helper it calls) and by the message's format. Where
several such sites give the same text (a bare "null argument"), the listing cannot tell which one answered: the case is marked * and counted for the
site with the fewest cases so far, so for starred sites "has a case" means "as many cases as sites give this text", to be read against the table.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_post_refusals.py
"""
from __future__ import annotations

import glob
import json
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

E_INVALID = -1
FUNCTION = re.compile(r"^(?:static |inline |template <[^>]*> )*(?:int|bool|size_t|double|void|PostRunTable|PlaneMap) (\w+)\(", re.M)
SITE = re.compile(r'fail\(MDPT_E_INVALID,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)')
RECORD_ENTRY = re.compile(r"mdpt_post_(guided|refocus|normals|shadows)")


def sites_of(path):
    """-> [(function, line, format)] of every fail( site, and {function: the functions it names}"""
    text = open(path).read()
    starts = [(m.start(), m.group(1)) for m in FUNCTION.finditer(text)]
    sites, calls = [], {}
    for k, (at, name) in enumerate(starts):
        body = text[at:starts[k + 1][0] if k + 1 < len(starts) else len(text)]
        calls[name] = set(re.findall(r"\b(\w+)\(", body)) - {name}
        for m in SITE.finditer(body):
            fmt = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1)))
            sites.append((name, text.count("\n", 0, at + m.start()) + 1, fmt))
    return sites, calls


def matches(fmt, message):
    pattern = re.sub(r"%(?:lld|zu|d|g|s|\.0f)", "\0", fmt)
    return re.fullmatch(".*".join(re.escape(part) for part in pattern.split("\0")), message, re.S) is not None


def main():
    from muggled_dpt_amd import native
    from tests import post_refusal_cases as table

    dirty = subprocess.run(["git", "status", "--porcelain", "--", "muggled_dpt_amd/csrc", "include"], cwd=REPO, capture_output=True, text=True, check=True).stdout
    if dirty.strip():
        sys.exit("csrc/ or include/ differ from the commit: the library would not be that commit's\n" + dirty)
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True, check=True).stdout.strip()
    lib = native.load()

    sources = sorted(glob.glob(os.path.join(native.CSRC, "mdpt_post*.cpp")) + glob.glob(os.path.join(native.CSRC, "mdpt_post_checks.h")))
    sites, calls = [], {}
    for path in sources:
        s, c = sites_of(path)
        sites += [(os.path.basename(path),) + x for x in s]
        calls.update(c)

    def reach(entry):  # the entry point and the helpers it calls, helpers of helpers included
        seen, todo = set(), [entry]
        while todo:
            f = todo.pop()
            if f not in seen and f in calls:
                seen.add(f)
                todo += calls[f]
        return seen

    refusals, covered, bad = {}, {}, []
    for name, entry, changed in table.CASES:
        rc, message, _ = table.run(lib, entry, changed)
        if rc != E_INVALID:
            bad.append(f"{name}: returned {rc} ({message!r}), not MDPT_E_INVALID")
            continue
        assert name not in refusals, name
        refusals[name] = [rc, message]
        within = reach(entry)
        hit = [s for s in sites if s[1] in within and matches(s[3], message)]
        if not hit:
            bad.append(f"{name}: no fail( site of {entry} gives {message!r}")
        else:  # a message that several reachable sites give (a bare "null argument") goes to the one with the fewest cases so far, marked *
            site = min(hit, key=lambda s: (len(covered.get(s, [])), s[2]))
            covered.setdefault(site, []).append(name + ("*" if len(hit) > 1 else ""))
    accepted = {}
    for name, entry, changed in table.ACCEPTED:
        rc, message, value = table.run(lib, entry, changed)
        if rc != 0:
            bad.append(f"{name}: an accepted query returned {rc} ({message!r})")
        accepted[name] = [rc, value]

    print("site (line) -> cases")
    entries = sorted(f for f in calls if f.startswith("mdpt_post_"))
    for site in sites:
        file, function, line, fmt = site
        must = function.startswith("check_") or RECORD_ENTRY.match(function) or "scratch of %zu bytes" in fmt or not function.startswith("mdpt_post_")
        names = covered.get(site, [])
        print(f"  {file}:{line} {function}: {fmt!r} -> {', '.join(names) if names else '-'}")
        if must and not names:
            bad.append(f"{file}:{line} {function}: no case gives {fmt!r}")
    for entry in entries:
        if not any(e == entry for _, e, _ in table.CASES):
            bad.append(f"{entry}: no refusal case")
    if bad:
        sys.exit("NOT written:\n  " + "\n  ".join(bad))
    out = os.path.join(REPO, "tests", "golden", "post_refusals.json")
    with open(out, "w") as fh:
        json.dump({"header": {"commit": commit, "sources": [os.path.basename(p) for p in sources], "entry_points": len(entries), "refusals": len(refusals),
                              "accepted": len(accepted)}, "refusals": refusals, "accepted": accepted}, fh, indent=0)
        fh.write("\n")
    print(f"wrote {len(refusals)} refusals and {len(accepted)} accepted queries of {len(entries)} entry points at {commit} to {out}")


if __name__ == "__main__":
    main()
