"""TEST INFRASTRUCTURE -- the REFERENCE's extension ops as a CPU module, built from its sources where they lie.

`ref_ops()` returns the module `oracle/_ref/pconv_ref_ops*.so` (building it on first use when the reference tree is
present) or None.  The recipe reads the reference's extension/*.cu, deletes each `<<< ... >>>` launch configuration
(so a kernel launch becomes a plain call), writes those copies under oracle/_ref/ref_ops_src/ (git-ignored, never
committed) and compiles them with g++ against oracle/ref_shim/ (our stand-ins for the CUDA headers) and the installed
torch headers, with floating-point contraction off.  One thread walks each grid-stride loop, so every such kernel
computes what the reference computes.

The masked convolution (entropy_conv_cuda_v2.cu) is the one file whose kernels are blocks of 128 cooperating threads
(shared memory, __syncthreads, warp shuffles).  For it alone a launch `k<<<grid, block, smem, stream>>>(args);`
becomes `shim_coop::launch(grid, block, smem, stream, [&] { k(args); });` and the file is compiled with
-DSHIM_COOPERATIVE: oracle/ref_shim/coop_launch.{h,cpp} then run the blocks one after another, each as `block`
fibers with per-thread indices, a warp of 32, a real barrier and a real shuffle.  Contraction stays off for it too.
oracle/ref_shim/coop_selfcheck.cu, kernels of our own, goes the same way and checks that launcher.
`make -C oracle ref_ops` runs the same recipe.
"""
import glob
import importlib.util
import os
import re
import subprocess
import sys
import sysconfig
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("PCONV_REFERENCE", "/root/reference")   # the reference tree (build container only)
OUT = os.path.join(HERE, "_ref")
NAME = "pconv_ref_ops"
MAX_JOBS = 8
LAUNCH = re.compile(r"<<\s?<[^;\n]*?>>\s?>")
COOPERATIVE = ("entropy_conv_cuda_v2",)      # files of the reference whose kernels are cooperating blocks
SELFCHECK = os.path.join(HERE, "ref_shim", "coop_selfcheck.cu")
KERNEL_NAME = re.compile(r"[A-Za-z_]\w*(\s*<[^<>;(){}]*>)?\s*$")
_mod = None


def _module_path():
    return os.path.join(OUT, NAME + sysconfig.get_config_var("EXT_SUFFIX"))


def _flags():
    import torch
    from torch.utils import cpp_extension
    inc = [os.path.join(HERE, "ref_shim"), os.path.join(REFERENCE, "extension")]
    inc += cpp_extension.include_paths() + [sysconfig.get_paths()["include"]]
    cflags = ["-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w", "-DTORCH_EXTENSION_NAME=" + NAME,
              "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI)]
    for d in inc:
        cflags += ["-I", d]
    libdir = os.path.join(os.path.dirname(torch.__file__), "lib")
    ldflags = ["-shared", "-L" + libdir, "-Wl,-rpath," + libdir, "-ltorch_python", "-ltorch", "-ltorch_cpu", "-lc10"]
    return cflags, ldflags


def cooperative_launches(text):
    """`name<t...><<<config>>>(args);` -> `shim_coop::launch(config, [&] { name<t...>(args); });`, everywhere"""
    out, pos = [], 0
    while True:
        i = text.find("<<<", pos)
        if i < 0:
            break
        j = text.index(">>>", i)
        tail = max(pos, i - 200)
        m = KERNEL_NAME.search(text, tail, i)
        name_at = m.start()
        k = text.index("(", j)
        assert not text[j + 3:k].strip(), text[i:k + 1]
        depth, close = 0, k
        while True:
            depth += {"(": 1, ")": -1}.get(text[close], 0)
            if depth == 0:
                break
            close += 1
        assert text[close + 1:].lstrip().startswith(";"), text[i:close + 2]
        out.append(text[pos:name_at])
        out.append("shim_coop::launch(%s, [&] { %s%s; })" % (text[i + 3:j].strip(), text[name_at:i].strip(),
                                                             text[k:close + 1]))
        pos = close + 1
    out.append(text[pos:])
    return "".join(out)


def build(jobs=MAX_JOBS, verbose=False):
    """compile every extension/*.cu of the reference (and its string2class.cc) with our binding into the module;
    raises on a compiler error, returns the module's path"""
    ext = os.path.join(REFERENCE, "extension")
    if not os.path.isdir(ext):
        raise RuntimeError("reference tree absent: " + ext)
    src_dir, obj_dir = os.path.join(OUT, "ref_ops_src"), os.path.join(OUT, "ref_ops_obj")
    os.makedirs(src_dir, exist_ok=True)
    os.makedirs(obj_dir, exist_ok=True)
    sources, cooperative = [], set()
    for cu in sorted(glob.glob(os.path.join(ext, "*.cu"))) + [SELFCHECK]:
        with open(cu) as f:
            text = f.read()
        dst = os.path.join(src_dir, os.path.basename(cu)[:-3] + ".cpp")
        if cu == SELFCHECK or os.path.basename(cu)[:-3] in COOPERATIVE:
            text = cooperative_launches(text)
            cooperative.add(dst)
        else:
            text = LAUNCH.sub("", text)
        if not os.path.exists(dst) or open(dst).read() != text:
            with open(dst, "w") as f:
                f.write(text)
        sources.append(dst)
    sources += [os.path.join(ext, "string2class.cc"), os.path.join(HERE, "ref_ops_bind.cpp"),
                os.path.join(HERE, "ref_shim", "coop_launch.cpp")]
    cflags, ldflags = _flags()
    cxx = os.environ.get("CXX", "g++")

    shim = glob.glob(os.path.join(HERE, "ref_shim", "**", "*.h"), recursive=True) + glob.glob(os.path.join(ext, "*.h*"))
    shim.append(os.path.abspath(__file__))
    newest_header = max(os.path.getmtime(h) for h in shim)

    def compile_one(src):
        obj = os.path.join(obj_dir, os.path.splitext(os.path.basename(src))[0] + ".o")
        if os.path.exists(obj) and os.path.getmtime(obj) > max(os.path.getmtime(src), newest_header):
            return src, obj, 0, ""
        extra = ["-DSHIM_COOPERATIVE"] if src in cooperative else []
        r = subprocess.run([cxx] + cflags + extra + ["-c", src, "-o", obj], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT)
        if verbose:
            print(("ok    " if r.returncode == 0 else "FAIL  ") + os.path.basename(src), flush=True)
        return src, obj, r.returncode, r.stdout.decode(errors="replace")

    with ThreadPoolExecutor(max(1, min(int(jobs), MAX_JOBS))) as pool:
        done = list(pool.map(compile_one, sources))
    bad = [(s, log) for s, _, rc, log in done if rc != 0]
    if bad:
        raise RuntimeError("\n".join("%s:\n%s" % (s, log[-4000:]) for s, log in bad))
    objs = [o for _, o, _, _ in done]
    if os.path.exists(_module_path()) and os.path.getmtime(_module_path()) > max(os.path.getmtime(o) for o in objs):
        return _module_path()
    tmp = _module_path() + ".tmp"
    r = subprocess.run([cxx] + [o for _, o, _, _ in done] + ldflags + ["-o", tmp], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError(r.stdout.decode(errors="replace")[-4000:])
    os.replace(tmp, _module_path())
    return _module_path()


def ref_ops():
    """the reference's ops on the CPU (a Python module with the class names of oracle.pconv_cpu), or None where
    neither a built module nor the reference tree exists"""
    global _mod
    if _mod is None:
        path = _module_path()
        if os.path.isdir(os.path.join(REFERENCE, "extension")):
            build()          # compiles what is missing or older than its source, the shim or the binding
        elif not os.path.exists(path):
            return None
        import torch  # noqa: F401  (libtorch must be loaded first)
        spec = importlib.util.spec_from_file_location(NAME, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _mod = mod
    return _mod


if __name__ == "__main__":
    print(build(verbose=True))
    sys.exit(0)
