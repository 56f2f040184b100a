"""tests/launch_cap_cases.py names every __global__ kernel of the data-plane files with its launch class, and for a capped
launch the line and the test that crosses it: a kernel added without an entry fails here by name."""
import ast
import os
import re

import launch_cap_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clairvoyante_amd", "csrc")
# __global__ ... void NAME(   -- with __launch_bounds__(...) on either side of `void`, and a template line in front
KERNEL = re.compile(r"__global__\s+(?:__launch_bounds__\s*\((?:[^()]|\([^()]*\))*\)\s*)?void\s+"
                    r"(?:__launch_bounds__\s*\((?:[^()]|\([^()]*\))*\)\s*)?(\w+)\s*\(")


def _kernels(stem):
    return KERNEL.findall(open(os.path.join(CSRC, stem + ".hip")).read())


def test_the_expression_reads_every_spelling():
    text = ("__global__ void a(int x)\n__global__ __launch_bounds__(W * cvi::LANES) void b(\ntemplate <bool W>\n__global__ __launch_bounds__(256) "
            "void c(int)\n__global__ void __launch_bounds__(E * 64)\nd(const int *p)\n__global__ __launch_bounds__(f(2)) void e (")
    assert KERNEL.findall(text) == ["a", "b", "c", "d", "e"]


def test_every_device_file_is_listed_once():
    """a .hip file is the inventory's (FILES) or the compute plane's (OUTSIDE): a new one cannot go by unlisted"""
    stems = sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert len(set(L.FILES)) == len(L.FILES) and len(set(L.OUTSIDE)) == len(L.OUTSIDE)
    both = sorted(set(L.FILES) & set(L.OUTSIDE))
    unlisted = sorted(set(stems) - set(L.FILES) - set(L.OUTSIDE))
    gone = sorted((set(L.FILES) | set(L.OUTSIDE)) - set(stems))
    assert not both, "in FILES and in OUTSIDE of tests/launch_cap_cases.py: %s" % ", ".join(both)
    assert not unlisted, "device files neither in FILES nor in OUTSIDE of tests/launch_cap_cases.py: %s" % ", ".join(s + ".hip" for s in unlisted)
    assert not gone, "listed in tests/launch_cap_cases.py, missing in csrc: %s" % ", ".join(gone)


def test_every_kernel_has_an_entry_and_every_entry_a_kernel():
    found = {}
    for stem in L.FILES:
        names = _kernels(stem)
        assert names, stem
        assert open(os.path.join(CSRC, stem + ".hip")).read().count("__global__") == len(names), "%s: a __global__ the expression misses" % stem
        for n in names:
            assert n not in found, "%s is defined in %s and in %s" % (n, found.get(n), stem)
            found[n] = stem
    missing = sorted(set(found) - set(L.KERNELS))
    stale = sorted(set(L.KERNELS) - set(found))
    assert not missing, "kernels without an entry in tests/launch_cap_cases.py: %s" % ", ".join(missing)
    assert not stale, "entries without a kernel: %s" % ", ".join(stale)
    for n, e in L.KERNELS.items():
        assert e["file"] == found[n], n


def _tests_of(path):
    tree = ast.parse(open(os.path.join(ROOT, path)).read())
    return {f.name for f in tree.body if isinstance(f, ast.FunctionDef) and f.name.startswith("test")}


def test_entries_are_whole_and_their_tests_exist():
    seen = {}
    for n, e in L.KERNELS.items():
        assert e["class"] in ("uncapped", "fixed", "capped"), n
        if e["class"] == "uncapped":
            assert e["grid"], n
        elif e["class"] == "fixed":
            assert e["note"], n
        else:
            assert e["item"] and isinstance(e["line"], int) and e["line"] > 0, n
            if e["test"] is None:
                assert len(e.get("why", "")) > 40, "%s: no test crosses its line and no reason is given" % n
            for t in [e["test"]] + e.get("also", []) if e["test"] else []:
                path, name = t.split("::")
                if path not in seen:
                    seen[path] = _tests_of(path)
                assert name in seen[path], "%s: %s does not exist" % (n, t)
    assert len(seen) >= 4


def test_the_lines_are_the_sources_constants():
    """the constants the lines are written from, read back from the sources"""
    src = lambda stem: open(os.path.join(CSRC, stem)).read()
    common = src("cv_dev_common.hpp")
    assert "int threads = 256, int max_grid = 4096" in common and L.GRID_FOR == 256 * 4096
    for stem, needles in (("cv_textparse.hip", ("INDEX_GRID = 2048", "PARSE_GRID = 2048", "PARSE_WAVES = 4", "FIND_GRID = 1024", "TILE_THREADS = 256")),
                          ("cv_eval.hip", ("EV_GRID = 256", "EV_THREADS = 256")),
                          ("cv_inflate_dev.hip", ("INFLATE_GRID = 4096", "INFLATE_WAVES = 4")),
                          ("cv_gzip_dev.hip", ("GRID = 4096", "WAVES = 4", "256 * 8")),
                          ("cv_blosc_dev.hip", ("DECODE_GRID = 8192", "DECODE_WAVES = 4")),
                          ("cv_blosc_pack_dev.hip", ("MAX_GRID = 1 << 20",)),
                          ("cv_beditems_dev.hip", ("blocks < 65536 ? blocks : 65536",)),
                          ("cv_bam_dev.hip", ("nwalk < 4096 ? nwalk : 4096",)),
                          ("cv_inflate_core.hpp", ("CRC_CHUNK = 1024",)),
                          ("cv_bgzf_deflate_dev.hip", ("MAX_GRID = 512", "cv_grid_for(members, 1, MAX_GRID)", "cv_grid_for(members, 1, 4096)")),
                          ("cv_vcfmerge_dev.hip", ("cv_grid_for((n + LANES - 1) / LANES, 1, 1 << 16)", "cv_grid_for(nrank, 1, 1024)")),
                          ("cv_vcfmerge_core.hpp", ("TILE_TEXT = 16 * 1024", "LANES = 64", "MAX_RANKS = 1 << 20", "POS_BITS = 40"))):
        text = src(stem)
        for needle in needles:
            assert needle in text, (stem, needle)
    K = L.KERNELS
    assert K["bd_compress"]["line"] == 512 and K["bd_assemble"]["line"] == 4096 and K["vw_backfill"]["line"] == 1024
    assert K["vm_gather"]["line"] == (1 << 16) * 64 == 4194304
