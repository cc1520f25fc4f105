"""Which object of the library defines which kernel (a kernel header is included by the unit that launches from it
and by no other).  The device compiler emits every static __global__ function a unit sees, launched from it or not, so a
kernel header that reaches a second unit shows up as a second definition: read off the kernel-descriptor symbols (<name>.kd)
of the gfx950 code object in every object file.  Symbol names only; no GPU."""
import os
import re
import shutil
import subprocess

import pytest

from robotoc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "robotoc_amd", "csrc", "build")


def _runtime_units():
    """the units of the host runtime as the Makefile links them: the names on its RT_OBJS line"""
    with open(os.path.join(ROOT, "robotoc_amd", "csrc", "Makefile")) as f:
        line = next(ln for ln in f if ln.startswith("RT_OBJS"))
    units = re.findall(r"\b(rtoc_capi|rt_\w+)\b", line)
    assert len(units) >= 14 and len(set(units)) == len(units), line
    return units


RUNTIME_UNITS = _runtime_units()
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return shutil.which(name)


def _kernels(obj, tools, tmp):
    """demangled names of the kernels the gfx950 code object inside `obj` defines"""
    base = os.path.join(str(tmp), os.path.basename(obj))
    if ".hip_fatbin" not in subprocess.check_output([tools["llvm-readobj"], "--sections", obj], text=True):  # a unit without device code
        return []
    subprocess.check_call([tools["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + base + ".fatbin", obj])
    subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + base + ".fatbin",
                           "--output=" + base + ".co"])
    if os.path.getsize(base + ".co") == 0:  # no device code at all
        return []
    out = subprocess.check_output([tools["llvm-readobj"], "--symbols", base + ".co"], text=True)
    names = sorted({ln.split()[1][:-3] for ln in out.splitlines() if ln.strip().startswith("Name: ") and ln.split()[1].endswith(".kd")})
    if not names:
        return []
    return subprocess.check_output(["c++filt"] + names, text=True).split("\n")[:len(names)]


@pytest.fixture(scope="module")
def kernels_by_object(tmp_path_factory):
    tools = {t: _tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readobj")}
    if not all(tools.values()):
        pytest.skip("ROCm's llvm tools are not installed")
    # the Makefile's objects: <unit>.o, shape_<nv>_<nu>_<ns>_<nw0>_<nw1>.o
    stems = [u + ".o" for u in RUNTIME_UNITS] + ["shape_%d_%d_%d_" % s for s in capi.compiled_shapes()]

    def find():
        have = sorted(os.listdir(BUILD)) if os.path.isdir(BUILD) else []
        return [next((os.path.join(BUILD, h) for h in have if h.endswith(".o") and h.startswith(s)), None) for s in stems]

    paths = find()
    if None in paths:  # a tree whose library came without its objects: build them
        capi.build(force=True)
        paths = find()
    assert None not in paths, "the build left no object for %r" % [s for s, p in zip(stems, paths) if p is None]
    tmp = tmp_path_factory.mktemp("code_objects")
    return {os.path.basename(p): _kernels(p, tools, tmp) for p in paths}


def test_every_runtime_kernel_is_defined_in_one_unit(kernels_by_object):
    where = {}
    for unit in RUNTIME_UNITS:
        for k in kernels_by_object[unit + ".o"]:
            where.setdefault(k, []).append(unit)
    assert where, "no kernel found in any runtime object"
    twice = {k: u for k, u in where.items() if len(u) != 1}
    assert not twice, "kernels defined in more than one runtime unit: %r" % twice


def test_a_shape_object_defines_template_instantiations_only(kernels_by_object):
    shapes = {o: ks for o, ks in kernels_by_object.items() if o.startswith("shape_")}
    assert len(shapes) == len(capi.compiled_shapes())
    for o, ks in shapes.items():
        assert ks, o + " defines no kernel"
        plain = [k for k in ks if "<" not in k]
        assert not plain, "%s carries runtime kernels: %r" % (o, plain)


def test_units_that_launch_one_kernel_of_their_own_or_none(kernels_by_object):
    capi_k = kernels_by_object["rtoc_capi.o"]
    assert capi_k and all("stream_probe_kernel<" in k for k in capi_k), capi_k
    assert kernels_by_object["rt_shapes.o"] == []
    solve_k = kernels_by_object["rt_solve.o"]
    assert len(solve_k) == 1 and "mask_converged_kernel" in solve_k[0], solve_k
