"""The device inflate without a device: the decoder of mgp_inflate_core.h run on the host
under the sanitizers (a stand-alone program, a child process), the ingest hook of
libmgphost.so driven by a small C inflater that calls zlib, and the bindings' refusals."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import inflate_corpus as ic

ROOT = Path(__file__).resolve().parent.parent
COLS = ("start", "bc", "tlen", "flag", "mapq", "span", "rec_off", "payload")


# ---------------------------------------------------------------------------
# the core under the sanitizers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core_program(tmp_path_factory):
    """tests/inflate_core_main.cpp with mgp_inflate_core.h, -fsanitize=address,undefined."""
    exe = tmp_path_factory.mktemp("inflate_core") / "inflate_core_main"
    cxx = shutil.which("g++") or "c++"
    # (the sanitizers' runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", f"-I{ROOT / 'mgatk2_amd' / 'csrc'}", str(ROOT / "tests" / "inflate_core_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def run_core(exe, cases, tmp_path, name):
    path = tmp_path / f"{name}.bin"
    ic.write_corpus_file(path, cases)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout[-3000:], r.stderr[-3000:])
    assert f"{len(cases)} cases" in r.stdout and " 0 failed" in r.stdout, r.stdout[-2000:]


def test_core_valid_streams_bit_equal(core_program, tmp_path):
    """Every valid stream (zlib's, the hand-made far match, libdeflate's BAM blocks at levels
    1, 6 and 9) gives status 0 and zlib's bytes, with the guards around the flush intact."""
    cases = list(ic.valid_cases()) + list(ic.odd_cases()) + ic.bam_cases(tmp_path)
    assert len(cases) > 35
    run_core(core_program, cases, tmp_path, "valid")


def test_core_invalid_streams_give_their_status(core_program, tmp_path):
    """Every invalid stream gives its status (1 invalid, 2 size / truncated) and writes nothing."""
    cases = list(ic.invalid_cases())
    assert [c[3] for c in cases] == [1, 1, 2, 1, 1, 1, 1, 2, 2, 2]
    run_core(core_program, cases, tmp_path, "invalid")


def test_core_mutations_follow_zlib(core_program, tmp_path):
    """20,000 single-byte and single-bit mutations of the valid streams: no sanitizer report,
    status 0 exactly when zlib decodes to exactly isize bytes and reaches the end of the
    stream, and then the same bytes."""
    cases = ic.mutations(20000)
    n_ok = sum(1 for c in cases if c[3] == ic.OK)
    assert 1000 < n_ok < 19000  # (both verdicts are well represented)
    run_core(core_program, cases, tmp_path, "mutations")


# ---------------------------------------------------------------------------
# the hook of libmgphost.so, with a C inflater that calls zlib
# ---------------------------------------------------------------------------
HOOK_C = r"""
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
typedef struct { int mode; int calls; int allocs; int releases; int64_t blocks; } hook_state;
static hook_state *g_state;
int hook_run(void *ctx, const uint8_t *src, int64_t src_bytes, int64_t n_blocks, const uint64_t *coff,
             const uint32_t *clen, const uint32_t *isize, const uint64_t *out_off, uint8_t *out, int64_t out_bytes,
             int32_t *status) {
    hook_state *st = (hook_state *)ctx;
    st->calls++;
    st->blocks += n_blocks;
    if (st->mode == 3) return -1;
    for (int64_t i = 0; i < n_blocks; ++i) {
        if (coff[i] + clen[i] > (uint64_t)src_bytes || out_off[i] + isize[i] > (uint64_t)out_bytes) return -2;
        z_stream z;
        memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK) return -3;
        z.next_in = (Bytef *)(src + coff[i]);
        z.avail_in = clen[i];
        z.next_out = out + out_off[i];
        z.avail_out = isize[i];
        int rc = inflate(&z, Z_FINISH);
        status[i] = (rc == Z_STREAM_END && z.avail_out == 0) ? 0 : 1;
        inflateEnd(&z);
    }
    if (st->mode == 1 && n_blocks > 1) status[n_blocks / 2] = 1;
    if (st->mode == 2 && out_bytes > 100) out[out_bytes / 2] ^= 0x10;
    return 0;
}
void hook_bind(hook_state *st) { g_state = st; }
void *hook_alloc(int64_t bytes) { if (g_state) g_state->allocs++; return malloc(bytes > 0 ? (size_t)bytes : 1); }
void hook_release(void *p) { if (g_state) g_state->releases++; free(p); }
const char *hook_message(void) { return "the test hook refuses"; }
"""


class HookState(C.Structure):
    _fields_ = [("mode", C.c_int), ("calls", C.c_int), ("allocs", C.c_int), ("releases", C.c_int),
                ("blocks", C.c_int64)]


@pytest.fixture(scope="module")
def hook(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_hook")
    (d / "hook.c").write_text(HOOK_C)
    so = d / "libhook.so"
    subprocess.run([shutil.which("gcc") or "cc", "-O1", "-std=c11", "-fPIC", "-shared", str(d / "hook.c"), "-o",
                    str(so), "-lz"], check=True)
    return C.CDLL(str(so))


@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("inflate_bam") / "r.bam"
    names = ic.write_test_bam(path, 6)
    return path, names


def set_hook(bam, hook, state, allocators: bool):
    from mgatk2_amd.bam import mgp_bam_inflater

    addr = lambda f: C.cast(f, C.c_void_p).value
    hook.hook_bind(C.byref(state))
    h = mgp_bam_inflater(addr(hook.hook_run), C.addressof(state), addr(hook.hook_alloc) if allocators else None,
                         addr(hook.hook_release) if allocators else None, addr(hook.hook_message))
    assert bam.lib.mgp_bam_set_inflater(bam._h, C.byref(h)) == 0


def read_all(bam, names):
    soa = bam.read_soa("chrM", names)
    return {k: np.array(getattr(soa, k)) for k in COLS}


def stream_all(bam, names, batch=700):
    from mgatk2_amd.bam import StreamSlot

    parts = []
    slot = StreamSlot(batch, batch * 64 + 256 * (len(names) + 1) + (1 << 20))
    with bam.stream("chrM", names) as st:
        while st.next_into(slot):
            v = slot.soa()
            parts.append({k: getattr(v, k).copy() for k in COLS})
    return parts


@pytest.mark.parametrize("allocators", [False, True])
def test_hook_gives_the_host_inflates_arrays(hook, small_bam, allocators):
    """read_soa and stream through a hook that inflates with zlib equal the run without the
    hook, array for array, with and without the hook's allocators; NULL restores the host path."""
    from mgatk2_amd.bam import BamFile

    path, names = small_bam
    with BamFile(path) as bam:
        want = read_all(bam, names)
        want_parts = stream_all(bam, names)
    assert want["start"].shape[0] == 3000 and len(want_parts) > 2
    state = HookState()
    with BamFile(path, n_threads=3) as bam:
        set_hook(bam, hook, state, allocators)
        got = read_all(bam, names)
        calls = state.calls
        assert calls >= 1 and state.blocks >= 2
        parts = stream_all(bam, names)
        assert state.calls > calls
        first, checked = bam.find_tag("chrM", "CB", 1001)
        assert (first, checked) == (0, 1001) or first >= 0
        assert sum(bam.count_tag("chrM").values()) > 0
        assert (state.allocs > 0) == allocators
        for k in COLS:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert len(parts) == len(want_parts)
        for a, b in zip(parts, want_parts):
            for k in COLS:
                np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        assert bam.lib.mgp_bam_set_inflater(bam._h, None) == 0
        calls = state.calls
        back = read_all(bam, names)
        assert state.calls == calls  # (the host path again)
        for k in COLS:
            np.testing.assert_array_equal(back[k], want[k], err_msg=k)
    assert state.allocs == state.releases


@pytest.mark.parametrize("mode,text", [(1, "BGZF inflate/CRC error"), (2, "BGZF inflate/CRC error"),
                                       (3, "the test hook refuses")])
def test_hook_errors_are_errors(hook, small_bam, mode, text):
    """A flipped status and a corrupted output byte (the CRC check survives the hook) give the
    host path's inflate/CRC error; a hook returning -1 gives an error with its message. Nothing
    falls back to the host inflate."""
    from mgatk2_amd.bam import BamFile
    from mgatk2_amd.exceptions import BAMReadError

    path, names = small_bam
    state = HookState(mode=mode)
    with BamFile(path) as bam:
        set_hook(bam, hook, state, False)
        with pytest.raises(BAMReadError, match=text):
            bam.read_soa("chrM", names)
        with pytest.raises(BAMReadError, match=text):
            stream_all(bam, names)
    assert state.calls >= 2


def test_hook_arguments_are_checked(hook, small_bam):
    from mgatk2_amd.bam import BamFile, mgp_bam_inflater

    path, _ = small_bam
    with BamFile(path) as bam:
        assert bam.lib.mgp_bam_set_inflater(bam._h, C.byref(mgp_bam_inflater())) != 0  # no run function
        addr = lambda f: C.cast(f, C.c_void_p).value
        half = mgp_bam_inflater(addr(hook.hook_run), None, addr(hook.hook_alloc), None, None)
        assert bam.lib.mgp_bam_set_inflater(bam._h, C.byref(half)) != 0  # alloc without release


# ---------------------------------------------------------------------------
# bindings, refusals without a device, the option
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ("mgp_bgzf_inflate", "mgp_inflater_create", "mgp_inflater_destroy", "mgp_inflater_run",
               "mgp_inflater_host_alloc", "mgp_inflater_host_release", "mgp_inflater_times")


def test_new_symbols_are_exported():
    from mgatk2_amd import engine
    from mgatk2_amd.bam import host_library

    lib = engine.load_library()
    for s in NEW_SYMBOLS:
        assert s in engine.ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.mgp_abi_version() == 7
    assert hasattr(host_library(), "mgp_bam_set_inflater")
    assert hasattr(engine, "inflate_bgzf") and hasattr(engine, "Inflater")


def test_arguments_refused_without_a_device():
    """Every refusal of the arguments is made before any allocation or launch: here, where
    there is no device, each is MGP_E_INVALID with its own message."""
    from mgatk2_amd import engine
    from mgatk2_amd.exceptions import InvalidInputError

    s = ic.valid_cases()[1][1]  # the 1-byte stream
    src = np.frombuffer(s + s, np.uint8)
    out = np.zeros(16, np.uint8)

    def call(coff, clen, isize, ooff, o=out):
        return engine.inflate_bgzf(src, coff, clen, isize, ooff, o)

    with pytest.raises(InvalidInputError, match="overlapping"):
        call([0, len(s)], [len(s)] * 2, [4, 4], [0, 3])
    with pytest.raises(InvalidInputError, match="overlapping"):
        call([0, len(s)], [len(s)] * 2, [1, 1], [8, 0])  # unsorted
    with pytest.raises(InvalidInputError, match="65536"):
        call([0], [len(s)], [65537], [0], np.zeros(70000, np.uint8))
    with pytest.raises(InvalidInputError, match="outside src"):
        call([len(s)], [len(s) + 1], [1], [0])
    with pytest.raises(InvalidInputError, match="outside src"):
        call([2 * len(s) + 1], [0], [1], [0])
    with pytest.raises(InvalidInputError, match="outside out"):
        call([0], [len(s)], [1], [16])
    with pytest.raises(InvalidInputError, match="outside out"):
        call([0], [len(s)], [17], [0])
    lib = engine.load_library()
    one = np.zeros(1, np.uint64)
    assert lib.mgp_bgzf_inflate(0, None, 4, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data,
                                out.ctypes.data, 16, one.ctypes.data) == engine.MGP_E_INVALID  # null src
    assert lib.mgp_bgzf_inflate(0, src.ctypes.data, 4, 1, None, None, None, None, out.ctypes.data, 16,
                                None) == engine.MGP_E_INVALID  # null arrays
    assert lib.mgp_bgzf_inflate(0, src.ctypes.data, 4, -1, None, None, None, None, out.ctypes.data, 16,
                                None) == engine.MGP_E_INVALID  # negative count
    assert lib.mgp_inflater_create(0, -1, 1, C.byref(C.c_void_p())) == engine.MGP_E_INVALID
    assert lib.mgp_inflater_run(None, None, 0, 0, None, None, None, None, None, 0, None) == engine.MGP_E_INVALID
    # no blocks: nothing is launched, nothing is needed
    assert lib.mgp_bgzf_inflate(0, None, 0, 0, None, None, None, None, None, 0, None) == 0


def test_option_in_every_command_and_config():
    from click.testing import CliRunner

    from mgatk2_amd import cli
    from mgatk2_amd.config import PipelineConfig

    for cmd in ("run", "tenx", "call"):
        r = CliRunner().invoke(cli.cli, [cmd, "--help"])
        assert r.exit_code == 0 and "--device-inflate" in r.output, cmd
    assert cli._variant_args(False, 5, 0.65, 0.01, False, 10, 1, device_inflate=True) == {"device_inflate": True}
    assert "device_inflate" not in cli._variant_args(False, 5, 0.65, 0.01, False, 10, 1)
    assert PipelineConfig().device_inflate is False
    cfg = PipelineConfig(device_inflate=True, inflate_device=2)
    assert cfg.device_inflate is True and cfg.inflate_device == 2


def test_keyword_reaches_the_config(tmp_path, monkeypatch):
    """run_pipeline(device_inflate=True) builds a PipelineConfig with the field set and the
    first of `devices` as the inflate's device."""
    from mgatk2_amd import pipeline

    seen = {}

    class Stop(Exception):
        pass

    def fake(**kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(pipeline, "MtDNAPipeline", fake)
    bfile = tmp_path / "b.tsv"
    bfile.write_text("AAAA-1\n")
    for kw, want in ((dict(device_inflate=True, devices=[3, 1]), (True, 3)), (dict(device=2), (False, 2))):
        with pytest.raises(Stop):
            pipeline.run_pipeline(str(tmp_path / "x.bam"), str(bfile), str(tmp_path / "o"), **kw)
        cfg = seen["config"]
        assert (cfg.device_inflate, cfg.inflate_device) == want
