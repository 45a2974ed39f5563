"""CPU: the dynamic symbol table of the built libartgpu.so against include/artgpu.h, without loading the library.
The C ABI is defined in several host files (artgpu_api.hip, one api_<stage>.hip for each stage that has left it, api_pipeline.hip, api_batch.hip);
an entry point that ends up outside `extern "C"` still links -- under its C++-mangled name -- and fails only at the first ctypes call.  Every
function the header declares must be defined under its plain name, and nothing named artgpu_* may be exported that the header does not declare.

The library is built with hidden visibility and the header's declarations stand inside a visibility pragma, so nothing is exported unless
include/artgpu.h declares it: the table may define nothing else either, but for what the toolchain puts there on its own (patterns below)."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")
HEADER = os.path.join(ROOT, "include", "artgpu.h")

# What hipcc and libstdc++ put into the table whatever the visibility flags say: (nm types, name)
TOOLCHAIN = [
    ("B", r"__hip_cuid_[0-9a-f]+"),                               # one marker per translation unit
    ("DV", r"_ZN6artgpu\d+\w+_kernel[EI]\w*"),                    # a __global__ function's handle object, which carries the kernel's name
    ("W", r"_ZN?St\w+"),                                          # std:: templates instantiated here (libstdc++ pins their visibility)
]


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)      # a comment may name a function with its parentheses
    text = re.sub(r"//[^\n]*", " ", text)
    return set(m.group(1) for m in re.finditer(r"\b(artgpu_\w+)\s*\(", text))


def _symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    return [(line.split()[-2], line.split()[-1]) for line in out.splitlines() if len(line.split()) >= 2]


def _defined():
    return set(name for _, name in _symbols())


def test_header_and_dynamic_symbols_agree():
    # the test pins what the build exports: a missing library or a missing nm is a failure, not a skip
    assert os.path.exists(LIB), "art_amd/libartgpu.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    assert shutil.which("nm") is not None, "no nm to read the dynamic symbol table"
    declared, defined = _declared(), _defined()
    assert len(declared) > 50, "the header's declarations were not found"
    missing = sorted(declared - defined)
    assert not missing, f"declared in include/artgpu.h, not defined (unmangled) in libartgpu.so: {missing}"
    undeclared = sorted(n for n in defined - declared if n.startswith("artgpu_"))
    assert not undeclared, f"exported by libartgpu.so, not declared in include/artgpu.h: {undeclared}"

    # ... and nothing else, but for the toolchain's own
    symbols = _symbols()
    assert len(symbols) > len(declared), "nm printed no table"
    leaked = sorted(f"{kind} {name}" for kind, name in symbols
                    if not (kind == "T" and name in declared) and not any(kind in kinds and re.fullmatch(pat, name) for kinds, pat in TOOLCHAIN))
    assert not leaked, ("libartgpu.so exports names that are neither entry points of include/artgpu.h nor the toolchain's: "
                        f"{leaked} -- every translation unit is compiled with -fvisibility=hidden -fvisibility-inlines-hidden (art_amd/csrc/Makefile), "
                        "and only the declarations of include/artgpu.h have default visibility")
