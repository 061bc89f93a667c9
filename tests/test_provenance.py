"""Counter provenance (CPU): the counters bench.py reports next to a live
measurement (roofline.traffic from FETCH_SIZE/WRITE_SIZE, valu from
SQ_INSTS_VALU) are read from committed rocprofv3 records, so they must belong
to the library being timed.  The Makefile compiles a hash of the receive
kernels' sources and compile command into the library (qpsk_kernel_hash());
profiles/summarize.py stores the profiled library's hash in each record and
bench.pmc_record() drops a record whose hash differs from the running one."""
import json
import os
import re
import shutil

import pytest

import bench
import singlecarrier_amd as sc

CSRC = os.path.join(os.path.dirname(sc.__file__), "csrc")


def _lib_built():
    if not os.path.exists(sc.LIB_PATH):
        pytest.skip("library not built")


def test_library_hash_is_the_sources_hash():
    _lib_built()
    assert re.fullmatch(r"[0-9a-f]{16}", sc.kernel_hash())
    assert sc.kernel_hash() == sc.kernel_source_hash()


def test_makefile_hashes_the_listed_sources():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    body = re.search(r"^KSRC\s*:=((?:.*\\\n)*.*)$", mk, re.M).group(1)
    assert tuple(body.replace("\\\n", " ").split()) == sc.KERNEL_SOURCES


def _kernel_unit_deps():
    """What qpsk_rx.hip, the kernels' translation unit, includes of the project
    (the compiler's own list): csrc-local names and include/ names."""
    import subprocess
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    inc = os.path.abspath(os.path.join(os.path.dirname(CSRC), "..", "include"))
    r = subprocess.run([hipcc, "--cuda-host-only", "-MM", "-std=c++17", f"-I{inc}", f"-I{CSRC}",
                        os.path.join(CSRC, "qpsk_rx.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    deps = [os.path.abspath(d) for d in r.stdout.split(":", 1)[1].replace("\\\n", " ").split()]
    local = {os.path.basename(d) for d in deps if os.path.dirname(d) == os.path.abspath(CSRC)}
    api = {os.path.basename(d) for d in deps if os.path.dirname(d) == inc}
    assert len(local) + len(api) == len(deps), deps
    return local, api


def _mk_list(name):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    body = re.search(rf"^{name}\s*:=((?:.*\\\n)*.*)$", mk, re.M).group(1)
    return body.replace("\\\n", " ").split()


def test_the_hash_covers_what_the_kernel_unit_includes_and_no_host_code():
    """KSRC / KHDR are exactly the files the kernels' translation unit is made
    from (its compile command: the tests on the hashed command below); the host
    side of the receive path (qpsk_rx_host.*) is none of them, so a host edit
    keeps the counter records."""
    local, api = _kernel_unit_deps()
    ksrc, khdr = _mk_list("KSRC"), _mk_list("KHDR")
    assert len(set(ksrc)) == len(ksrc) and set(ksrc) == local
    assert len(set(khdr)) == len(khdr) and all(h.startswith("$(INCDIR)/") for h in khdr)
    assert {h[len("$(INCDIR)/"):] for h in khdr} == api
    host = [f for f in os.listdir(CSRC) if f.startswith("qpsk_rx_host.")]
    assert host and not any(f in local or f in ksrc for f in host)


def test_a_host_file_byte_keeps_the_hash(tmp_path):
    cur = sc.kernel_source_hash()
    src = tmp_path / "csrc"
    shutil.copytree(CSRC, src, ignore=shutil.ignore_patterns("build"))
    assert sc.kernel_source_hash(str(src)) == cur
    for f in src.glob("qpsk_rx_host.*"):
        b = bytearray(f.read_bytes())
        b[len(b) // 2] ^= 1
        f.write_bytes(bytes(b))
    assert sc.kernel_source_hash(str(src)) == cur


def test_a_host_edit_rebuilds_only_the_host_object():
    """The host file as if just edited (make -W): its object is rebuilt, the
    kernels' translation unit is not compiled."""
    _lib_built()
    assert "qpsk_rx" not in _make("-n").stdout
    dry = _make("-n", "-W", "qpsk_rx_host.hip")
    assert dry.returncode == 0, dry.stderr
    assert "qpsk_rx_host.hip" in dry.stdout and "build/qpsk_rx_host.o" in dry.stdout
    assert "qpsk_rx.hip" not in dry.stdout and "build/qpsk_rx.o " in dry.stdout   # linked, not compiled


def _write_records(root, khash, nch=65536, nf=32):
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    json.dump({"channels": nch, "frames": nf, "hbm_bytes_per_launch": 123, "kernel_hash": khash,
               "source": "test"}, open(os.path.join(root, "profiles", "pmc_traffic.json"), "w"))
    json.dump({"channels": nch, "frames": nf, "valu_insts_per_launch": 456, "kernel_hash": khash,
               "source": "test"}, open(os.path.join(root, "profiles", "pmc_valu.json"), "w"))


def test_one_flipped_source_byte_drops_the_counters(tmp_path):
    """Records profiled with the current kernels are reported; after one byte
    of qpsk_rx.hip changes, the rebuilt library's hash differs and both
    records are dropped (traffic null, no measured valu).  So does one byte of
    a header the kernels moved to."""
    cur = sc.kernel_source_hash()
    _write_records(str(tmp_path), cur)
    p = bench.pmc_record("pmc_traffic.json", 65536, 32, "reference", cur, root=str(tmp_path))
    assert p is not None and p["hbm_bytes_per_launch"] == 123
    v = bench.valu_from_counters(bench.pmc_record("pmc_valu.json", 65536, 32, "reference", cur,
                                                  root=str(tmp_path)), 6e-3)
    assert v is not None and v["valu_insts_per_launch"] == 456 and v["kernel_hash"] == cur
    # the same sources with one byte flipped
    src = tmp_path / "csrc"
    shutil.copytree(CSRC, src, ignore=shutil.ignore_patterns("build"))
    f = src / "qpsk_rx.hip"
    b = bytearray(f.read_bytes())
    b[len(b) // 2] ^= 1
    f.write_bytes(bytes(b))
    new = sc.kernel_source_hash(str(src))
    assert new != cur
    for name in ("pmc_traffic.json", "pmc_valu.json"):
        assert bench.pmc_record(name, 65536, 32, "reference", new, root=str(tmp_path)) is None
    b[len(b) // 2] ^= 1   # back as it was
    f.write_bytes(bytes(b))
    assert sc.kernel_source_hash(str(src)) == cur
    f = src / "qpsk_rx_back.h"
    b = bytearray(f.read_bytes())
    b[len(b) // 2] ^= 1
    f.write_bytes(bytes(b))
    moved = sc.kernel_source_hash(str(src))
    assert moved != cur and moved != new
    assert bench.valu_from_counters(None, 6e-3) is None
    # a record without a hash (older profiles) is never reported either
    _write_records(str(tmp_path), None)
    assert bench.pmc_record("pmc_traffic.json", 65536, 32, "reference", cur, root=str(tmp_path)) is None


def test_record_of_another_workload_is_dropped(tmp_path):
    cur = sc.kernel_source_hash()
    _write_records(str(tmp_path), cur, nch=8192)
    assert bench.pmc_record("pmc_traffic.json", 65536, 32, "reference", cur, root=str(tmp_path)) is None
    assert bench.pmc_record("pmc_traffic.json", 8192, 32, "dec752", cur, root=str(tmp_path)) is None


def _make(*args):
    import subprocess
    inc = os.path.join(os.path.dirname(CSRC), "..", "include")
    return subprocess.run(["make", "-s", "--no-print-directory", "-C", CSRC, f"INCDIR={os.path.abspath(inc)}",
                           *args], capture_output=True, text=True)


def test_variant_flags_change_the_hash_and_force_a_rebuild():
    """a QPSK_VARIANT build must never keep the product's
    hash, a plain `make` after it must rebuild the product object, and knobs
    with quotes or spaces must hash as written (the flags reach the hash
    through a file, not the shell's quoting)."""
    _lib_built()
    base = _make("khash").stdout.strip()
    assert base == sc.kernel_hash()
    var = _make("khash", "QPSK_VARIANT=-DQPSK_FIR_NOMASK=1").stdout.strip()
    quoted = _make("khash", "QPSK_VARIANT=-DQPSK_RX_ATTR='__attribute__((amdgpu_num_vgpr(128)))'")
    assert quoted.returncode == 0 and re.fullmatch(r"[0-9a-f]{16}", quoted.stdout.strip())
    assert len({base, var, quoted.stdout.strip()}) == 3
    # the object depends on a per-hash stamp: with the variant's flags the
    # product object is out of date (dry run: nothing is built here)
    dry = _make("-n", "QPSK_VARIANT=-DQPSK_FIR_NOMASK=1")
    assert "qpsk_rx.hip" in dry.stdout and "QPSK_FIR_NOMASK" in dry.stdout
    assert "qpsk_rx.hip" not in _make("-n").stdout


def _syntax_only(*defs):
    import subprocess
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    inc = os.path.abspath(os.path.join(os.path.dirname(CSRC), "..", "include"))
    return subprocess.run([hipcc, "--cuda-host-only", "-fsyntax-only", "-std=c++17", f"-I{inc}", f"-I{CSRC}",
                           *defs, os.path.join(CSRC, "qpsk_rx.hip")], capture_output=True, text=True)


@pytest.mark.parametrize("knob", ["QPSK_FIR_SPLIT=2", "QPSK_HUNT_OVERLAP=0"])
def test_a_removed_knob_stops_the_build(knob):
    """The compile-time A/B knobs whose alternative branches are gone (DESIGN.md
    "Removed knobs") must not be accepted in silence: a variant script that
    still passes one would compare HEAD with itself.  qpsk_rx.hip refuses any
    of them with an #error that names it (QPSK_HUNT_OVERLAP was qpsk_hunt.h's,
    which qpsk_rx.hip includes); a knob that is still there passes."""
    r = _syntax_only(f"-D{knob}")
    assert r.returncode != 0
    assert "error:" in r.stderr and knob.split("=")[0] in r.stderr
    ok = _syntax_only("-DQPSK_STAMPS")
    assert ok.returncode == 0, ok.stderr


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(sc.__file__)))


def _compiles(dry):
    """The compile commands of a dry run, as argument lists."""
    import shlex
    return [shlex.split(l) for l in dry.stdout.splitlines() if " -c " in l]


@pytest.mark.parametrize("variant", [(), ("QPSK_VARIANT=-DQPSK_FIR_NOMASK=1",)])
def test_every_flag_of_the_kernel_compile_is_hashed(variant):
    """The compile command of build/qpsk_rx.o (dry run, the source as if just
    edited) is the hashed command (make kcmd) token for token, once the
    arguments that say where things lie are taken out: include directories,
    the output, the source, the dependency file, and the hash define itself.
    A flag written anywhere else on that command would fail this."""
    import shlex
    dry = _make("-n", "-W", "qpsk_rx.hip", "build/qpsk_rx.o", *variant)
    assert dry.returncode == 0, dry.stderr
    (cmd,) = _compiles(dry)
    rest, it = [], iter(cmd)
    for tok in it:
        if tok in ("-o", "-MF"):
            next(it)
        elif not (tok in ("-c", "-MMD", "-MP", "qpsk_rx.hip") or tok.startswith("-I")
                  or tok.startswith("-DQPSK_KERNEL_HASH=")):
            rest.append(tok)
    hashed = shlex.split(_make("kcmd", *variant).stdout)
    assert rest == hashed
    assert "-O3" in hashed and ("-DQPSK_FIR_NOMASK=1" in hashed) == bool(variant)


def test_the_hash_follows_the_flags_and_not_the_makefiles_text(tmp_path):
    cur = sc.kernel_source_hash()
    src = tmp_path / "csrc"
    shutil.copytree(CSRC, src, ignore=shutil.ignore_patterns("build"))
    mk = src / "Makefile"
    mk.write_text(mk.read_text() + "\n# one more object\nCSRC += extra.c\nREST += $(BUILD)/extra.o\n"
                  "$(BUILD)/extra.o: extra.c\n\t$(CC) $(CFLAGS) -c -o $@ $<\n")
    assert sc.kernel_source_hash(str(src)) == cur
    fl = src / "flags.mk"
    assert fl.read_text().count("-O3") == 1
    fl.write_text(fl.read_text().replace("-O3", "-O2"))
    assert sc.kernel_source_hash(str(src)) != cur


def test_every_source_file_is_one_object_of_the_library():
    objs = _make("restobj").stdout.split() + ["build/qpsk_rx.o"]
    files = [f for f in os.listdir(CSRC) if f.endswith((".hip", ".c"))]
    assert len(files) >= 15
    assert sorted(objs) == sorted(f"build/{os.path.splitext(f)[0]}.o" for f in files)


def test_the_tsan_library_compiles_every_source_of_the_product():
    """tests/callers builds its instrumented library from the product's
    Makefile: the same sources, none left out (dry runs, nothing is built)."""
    import subprocess
    tsan = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "tests", "callers"), "tsan"],
                          capture_output=True, text=True)
    assert tsan.returncode == 0, tsan.stderr
    prod = _make("-n", "-B")
    assert prod.returncode == 0, prod.stderr
    names = [sorted(os.path.basename(c[-1]) for c in _compiles(d)) for d in (tsan, prod)]
    assert names[0] == names[1] and len(names[1]) == len(set(names[1])) >= 15
    assert all("-fsanitize=thread" in c for c in _compiles(tsan))


def test_the_bit_exactness_flags_are_written_once():
    import glob
    files = (glob.glob(os.path.join(CSRC, "*")) + glob.glob(os.path.join(ROOT, "tests", "**", "Makefile"), recursive=True)
             + [f for f in glob.glob(os.path.join(ROOT, "profiles", "*.sh"))
                if not re.match(r"(r|round|call|session)\d+_", os.path.basename(f))]
             + glob.glob(os.path.join(ROOT, "profiles", "*.py")))
    flag = "-fno-gpu-flush-denormals-to-zero"
    holds = [os.path.relpath(f, ROOT) for f in files
             if os.path.isfile(f) and flag in open(f, errors="ignore").read()]
    assert holds == [os.path.join("singlecarrier_amd", "csrc", "flags.mk")]
