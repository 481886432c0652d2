"""ISA check of the headline kernel's store phase: cross-compiles the order-4, S = 16 translation
unit for gfx950 with build.py's flags and disassembles minsnap_fixed_persistent_kernel<4,16,false,false,NT> for both
store flavours.  No GPU needed; skipped where hipcc is absent.

Yardstick = the kernel before the store flavour became a template parameter: 384 global_store_dwordx4 (192 non-temporal
+ 192 ordinary, a run-time branch pair around each of the 192 logical stores) and 61 824 bytes of code."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGICAL_STORES = 192          # per kernel, both roles: 8 segments x 3 axes x 64 B x 64 lanes / (16 B x 64 lanes) each
PARENT_CODE_BYTES = 61824
KERNEL = "_ZN3csp6fixedk31minsnap_fixed_persistent_kernelILi4ELi16ELb0ELb0ELb%dEEEvNS_11GenericArgsEi"


def _build_module():
    spec = importlib.util.spec_from_file_location("csp_build", os.path.join(ROOT, "cs-pathplan_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tool(hipcc, name):
    for d in (os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin"), os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin")):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    b = _build_module()
    hipcc = b.HIPCC if os.path.exists(b.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not found")
    objdump, readelf = _tool(hipcc, "llvm-objdump"), _tool(hipcc, "llvm-readelf")
    if not objdump or not readelf:
        pytest.skip("llvm-objdump / llvm-readelf not found")
    tmp = tmp_path_factory.mktemp("isa")
    obj = str(tmp / "o4b.o")
    flags = [f for f in b.FLAGS if not f.startswith("-W")]
    r = subprocess.run([hipcc] + flags + ["--offload-device-only", "--no-gpu-bundle-output", "-Rpass-analysis=kernel-resource-usage",
                                          "-c", os.path.join(b.CSRC, "minsnap_fixed_o4b.hip"), "-o", obj],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-2000:]
    syms = subprocess.check_output([readelf, "-s", "-W", obj], universal_newlines=True)
    out = {}
    for nt in (0, 1):
        name = KERNEL % nt
        dis = subprocess.check_output([objdump, "-d", "--disassemble-symbols=" + name, obj], universal_newlines=True)
        m = re.search(r"^\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s.*\s%s$" % re.escape(name), syms, re.M)
        assert m, "kernel %s not in the object" % name
        # the remarks of one kernel: from its 'Function Name' line to the next one
        rem = r.stderr.split("Function Name: " + name + " ", 1)
        assert len(rem) == 2, "no resource-usage remarks for %s" % name
        rem = rem[1].split("Function Name:", 1)[0]
        res = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", rem)}
        out[nt] = {"asm": dis, "code_bytes": int(m.group(1)), "res": res}
    return out


@pytest.mark.parametrize("nt", [0, 1])
def test_one_store_flavour_per_instantiation(listing, nt):
    stores = [l for l in listing[nt]["asm"].splitlines() if re.match(r"\s*global_store_dwordx4\b", l)]
    n_nt = sum(1 for l in stores if re.search(r"\bnt\b", l.split("//")[0]))
    print("NT=%d: %d global_store_dwordx4, %d of them nt" % (nt, len(stores), n_nt))
    assert len(stores) == LOGICAL_STORES          # half the 384 of the run-time select
    assert n_nt == (LOGICAL_STORES if nt else 0)
    assert not re.search(r"^\s*flat_store", listing[nt]["asm"], re.M)


@pytest.mark.parametrize("nt", [0, 1])
def test_stores_take_a_scalar_base(listing, nt):
    """Every coefficient store is `global_store_dwordx4 v_off, v_data, s[base:base+1]`, and between the stores of a burst
    there is no 64-bit vector address arithmetic."""
    lines = [l.split("//")[0].strip() for l in listing[nt]["asm"].splitlines()]
    lines = [l for l in lines if l and not l.endswith(":")]
    idx = [i for i, l in enumerate(lines) if l.startswith("global_store_dwordx4")]
    assert all(re.search(r",\s*s\[\d+:\d+\]", lines[i]) for i in idx)
    # "Same burst" = at most 8 instructions apart (a store, its scalar base advance and its counted wait are 4).  The 192
    # stores leave in 24 bursts of 8, so 168 of the 191 neighbouring pairs are in-burst by construction; the floor keeps
    # the checks below from passing vacuously should the stores drift apart (a few pairs may have the next batch's LDS
    # reads scheduled between them).
    in_burst = sum(1 for a, b in zip(idx, idx[1:]) if b - a <= 8)
    print("NT=%d: %d of %d neighbouring store pairs are in-burst" % (nt, in_burst, len(idx) - 1))
    assert in_burst >= 150
    between = 0
    for a, b in zip(idx, idx[1:]):
        if b - a <= 8:
            between += sum(1 for l in lines[a + 1:b] if re.match(r"v_lshl_add_u64|v_add_co_u32|v_addc_co_u32", l))
    print("NT=%d: %d vector address instructions between stores of a burst" % (nt, between))
    assert between == 0
    # a burst is straight-line: no branch and no wait on vector memory between its stores (the counted lgkmcnt in
    # front of a store waits for that store's own LDS read only)
    broken = 0
    for a, b in zip(idx, idx[1:]):
        if b - a <= 8:
            broken += sum(1 for l in lines[a + 1:b] if l.startswith("s_cbranch") or ("s_waitcnt" in l and "vmcnt" in l))
    assert broken == 0


@pytest.mark.parametrize("nt", [0, 1])
def test_resources_and_code_size(listing, nt):
    res, code = listing[nt]["res"], listing[nt]["code_bytes"]
    print("NT=%d: code %d bytes, %s" % (nt, code, res))
    assert res["ScratchSize"] == 0
    assert res["VGPRs Spill"] == 0
    assert code < PARENT_CODE_BYTES
