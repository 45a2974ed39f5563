"""CPU: the dynamic symbol table of the built libartgpu.so against include/artgpu.h, without loading the library.
The C ABI is defined in several host files (artgpu_api.hip, one api_<stage>.hip for each stage that has left it, api_pipeline.hip, api_batch.hip);
an entry point that ends up outside `extern "C"` still links -- under its C++-mangled name -- and fails only at the first ctypes call.  Every
function the header declares must be defined under its plain name, and nothing named artgpu_* may be exported that the header does not declare.

Each of those files opens `extern "C"`, `artgpu::api` (hidden) and an anonymous namespace by hand; a function that lands in the wrong one
is exported by accident (an anonymous namespace inside `extern "C"` once exported 29 plain names).  So the table may define nothing else
either, but for what the toolchain generates (patterns below), the inline functions of the project's headers (by name) and the kernel
files' host interface (by name: tests/golden/abi_kernel_interface.txt)."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")
HEADER = os.path.join(ROOT, "include", "artgpu.h")
KERNEL_INTERFACE = os.path.join(ROOT, "tests", "golden", "abi_kernel_interface.txt")

# What hipcc, the linker and libstdc++ put into the table: (nm types, name)
TOOLCHAIN = [
    ("B", r"__hip_cuid_[0-9a-f]+"),                               # one marker per translation unit
    ("T", r"_init|_fini"),
    ("TW", r"_ZN6artgpu\d+__device_stub__\w+"),                   # a __global__ function's host stub ...
    ("DV", r"_ZN6artgpu\d+\w+_kernel[EI]\w*"),                    # ... and its handle, which carries the kernel's name
    ("VW", r"(_ZGV)?_Z(N|NK|ZN|ZNK)?(St|9__gnu_cxx)\w+"),         # std:: templates instantiated here, their static locals and guards
]
# Inline functions of the project's own headers that a translation unit emitted out of line, and their static locals: weak, not fixable
# with a brace or a `static` (kernels.h: dyn_lds_once, device_block_fits; paramcurve.h: pc_*; api_internal.h: artgpu_ctx's destructors)
INLINE = {
    "_Z12dyn_lds_oncePKvi", "_ZZ12dyn_lds_oncePKviE1m", "_ZZ12dyn_lds_oncePKviE4done", "_ZGVZ12dyn_lds_oncePKviE4done",
    "_Z17device_block_fitsii", "_ZZ17device_block_fitsiiE1m", "_ZZ17device_block_fitsiiE5known", "_ZZ17device_block_fitsiiE6lds_of",
    "_ZZ17device_block_fitsiiE6thr_of",
    "_ZN6artgpu6pc_p01Edd", "_ZN6artgpu6pc_p10Edd", "_ZN6artgpu7pc_initERNS_10ParamCurveEPKdi", "_ZN6artgpu8pc_baselEddd", "_ZN6artgpu8pc_pfullEdddd",
    "_ZN10artgpu_ctxD2Ev", "_ZN10artgpu_ctx11PipeRegionsI23artgpu_smoothing_regionED2Ev",
    "_ZN10artgpu_ctx11PipeRegionsI30artgpu_color_correction_regionED2Ev",
}


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


def _kernel_interface():
    return set(line.strip() for line in open(KERNEL_INTERFACE) if line.strip() and not line.startswith("#"))


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

    # ... and nothing else, but for the three allow-lists above
    interface = _kernel_interface()
    assert len(interface) > 100, "tests/golden/abi_kernel_interface.txt was not read"
    symbols = _symbols()
    assert len(symbols) > len(declared), "nm printed no table"
    leaked = sorted(f"{kind} {name}" for kind, name in symbols
                    if name not in declared and name not in INLINE and name not in interface
                    and not any(kind in kinds and re.fullmatch(pat, name) for kinds, pat in TOOLCHAIN))
    assert not leaked, ("libartgpu.so exports names that are neither entry points of include/artgpu.h, nor the toolchain's, nor the kernel files' "
                        f"interface: {leaked} -- a function of a host file belongs in `artgpu::api` (hidden), or is `static` / in an anonymous "
                        "namespace outside `extern \"C\"`; a new launcher of a kernel file is added to tests/golden/abi_kernel_interface.txt")
