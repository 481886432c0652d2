"""ISA check of the write-through flavour of the headline kernel: cross-compiles minsnap_fixed_o4d.hip
for gfx950 with build.py's flags and disassembles minsnap_fixed_persistent_wt_kernel<4,16,false,AUX>; the ordinary
instantiation minsnap_fixed_persistent_kernel<4,16,false,false,false> is compiled in the same test (minsnap_fixed_o4b.hip)
as the yardstick for the code size.  No GPU needed; skipped where hipcc is absent."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGICAL_STORES = 192          # per kernel, both roles: 8 pairs x (8 + 16) store instructions
AUX = 16                      # fixedk::SP_WT: the buffer store's cache bits, sc1
CACHE_BITS = {16: ("sc1",), 17: ("sc0", "sc1")}[AUX]
WT_KERNEL = "_ZN3csp6fixedk34minsnap_fixed_persistent_wt_kernelILi4ELi16ELb0ELi%dEEEvNS_11GenericArgsEi" % AUX
PLAIN_KERNEL = "_ZN3csp6fixedk31minsnap_fixed_persistent_kernelILi4ELi16ELb0ELb0ELb0EEEvNS_11GenericArgsEi"


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
    tmp = tmp_path_factory.mktemp("isa_wt")
    flags = [f for f in b.FLAGS if not f.startswith("-W")]
    jobs = {"wt": ("minsnap_fixed_o4d.hip", WT_KERNEL), "plain": ("minsnap_fixed_o4b.hip", PLAIN_KERNEL)}
    procs = {}
    for key, (src, _) in jobs.items():   # the two translation units compile side by side
        obj = str(tmp / (key + ".o"))
        procs[key] = (obj, subprocess.Popen([hipcc] + flags + ["--offload-device-only", "--no-gpu-bundle-output", "-Rpass-analysis=kernel-resource-usage",
                                                               "-c", os.path.join(b.CSRC, src), "-o", obj],
                                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True))
    out = {}
    for key, (obj, proc) in procs.items():
        _, err = proc.communicate()
        assert proc.returncode == 0, err[-2000:]
        name = jobs[key][1]
        syms = subprocess.check_output([readelf, "-s", "-W", obj], universal_newlines=True)
        dis = subprocess.check_output([objdump, "-d", "--disassemble-symbols=" + name, obj], universal_newlines=True)
        m = re.search(r"^\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s.*\s%s$" % re.escape(name), syms, re.M)
        assert m, "kernel %s not in the object" % name
        rem = err.split("Function Name: " + name + " ", 1)
        assert len(rem) == 2, "no resource-usage remarks for %s" % name
        rem = rem[1].split("Function Name:", 1)[0]
        res = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", rem)}
        lines = [l.split("//")[0].strip() for l in dis.splitlines()]
        out[key] = {"lines": [l for l in lines if l and not l.endswith(":")], "code_bytes": int(m.group(1)), "res": res}
    return out


def _stores(lines):
    return [i for i, l in enumerate(lines) if re.match(r"(buffer|global|flat|scratch)_store_dwordx4\b", l)]


def test_every_store_is_write_through(listing):
    lines = listing["wt"]["lines"]
    idx = _stores(lines)
    print("%d 16-byte stores" % len(idx))
    assert len(idx) == LOGICAL_STORES
    for i in idx:
        assert lines[i].startswith("buffer_store_dwordx4"), lines[i]
        bits = set(re.findall(r"\b(sc0|sc1|nt)\b", lines[i]))
        assert bits == set(CACHE_BITS), lines[i]
    assert not any(l.startswith("flat_store") for l in lines)
    assert not any(re.match(r"(global|scratch)_store", l) for l in lines)


def test_bursts_are_straight_line(listing):
    """Between the stores of a burst: no wait on vector memory, no branch, no vector address arithmetic (the lane
    offset is one VGPR, the displacement a scalar operand)."""
    lines = listing["wt"]["lines"]
    idx = _stores(lines)
    # as in tests/test_fixed_store_isa.py: 24 bursts of 8, so 168 of the 191 neighbouring pairs are in-burst by construction
    in_burst = [(a, b) for a, b in zip(idx, idx[1:]) if b - a <= 8]
    print("%d of %d neighbouring store pairs are in-burst" % (len(in_burst), len(idx) - 1))
    assert len(in_burst) >= 150
    broken = address = 0
    for a, b in in_burst:
        broken += sum(1 for l in lines[a + 1:b] if l.startswith("s_cbranch") or l.startswith("s_branch") or ("s_waitcnt" in l and "vmcnt" in l))
        address += sum(1 for l in lines[a + 1:b] if re.match(r"v_lshl_add_u64|v_add_co_u32|v_addc_co_u32|v_add_u32|v_readfirstlane", l))
    print("%d waits / branches, %d vector address instructions between stores of a burst" % (broken, address))
    assert broken == 0
    assert address == 0


def test_resources_and_code_size(listing):
    wt, plain = listing["wt"], listing["plain"]
    print("write-through: code %d bytes, %s; ordinary: code %d bytes" % (wt["code_bytes"], wt["res"], plain["code_bytes"]))
    assert wt["res"]["ScratchSize"] == 0
    assert wt["res"]["VGPRs Spill"] == 0
    assert wt["code_bytes"] <= plain["code_bytes"]
