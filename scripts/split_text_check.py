#!/usr/bin/env python3
"""Text check of a moves-only split of the C ABI host file: the non-blank lines of REV's artgpu_api.hip and
api_internal.h against those of the working tree's artgpu_api.hip, api_internal.h and every api_<stage>.hip REV did not have, as multisets.
Prints the two totals and each line that is only on one side, with its count: what is printed must be heads, braces, includes, headers,
banners and declarations -- never a line from inside a function body.

    python scripts/split_text_check.py HEAD~1
"""
import collections
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "art_amd/csrc"


def lines_of(text):
    return [l.rstrip() for l in text.split("\n") if l.strip()]


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    git = lambda *a: subprocess.run(["git", "-C", ROOT, *a], capture_output=True, text=True, check=True).stdout
    had = set(git("ls-tree", "--name-only", rev, CSRC + "/").split())
    old_files = [f"{CSRC}/artgpu_api.hip", f"{CSRC}/api_internal.h"]
    new_files = old_files + sorted(p for p in (os.path.relpath(q, ROOT) for q in glob.glob(os.path.join(ROOT, CSRC, "api_*.hip"))) if p not in had)
    old = collections.Counter(l for f in old_files for l in lines_of(git("show", f"{rev}:{f}")))
    new = collections.Counter(l for f in new_files for l in lines_of(open(os.path.join(ROOT, f)).read()))
    print(f"old: {sum(old.values())} non-blank lines in {len(old_files)} files of {rev}")
    print(f"new: {sum(new.values())} non-blank lines in {len(new_files)} files: " + " ".join(os.path.basename(f) for f in new_files))
    for title, d in (("only old", old - new), ("only new", new - old)):
        print(f"--- {title}: {sum(d.values())} lines")
        for l, c in sorted(d.items()):
            print(f"{c:3d}  {l}")


if __name__ == "__main__":
    main()
