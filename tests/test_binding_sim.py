"""CPU tier: the HOST LOGIC above the C ABI — table-shaped shim, per-thread contexts, picture registry, the VVenC binding (hooks, batching and replay, --SIMD=HIP
selection, picture -> device mapping) — exercised without a GPU.  The real reference encoder (oracle/_ref, compiled from /root/reference) runs with the binding installed
while tests/sim/libvvhip_sim.so, a TEST DOUBLE of the device library (device memory = host memory, kernels = the CPU oracle), is injected with LD_PRELOAD; the bitstream
must equal the CPU encoder's.  This says nothing about the HIP kernels (the -m gpu tests do); it pins everything around them, for every preset of BASELINE.json."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the small test clips have a handful of CTUs per encoder thread: take the whole-picture ALF statistics hook regardless of the binding's saturation rule (vvenc_hip_binding.cpp: alfPictureOn)
os.environ.setdefault("VVHIP_ALF_MIN_CTUS_PER_THREAD", "0")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import e2e_util  # noqa: E402
from test_e2e_bitstream import run, ALL_TABLES, BATCHED_SITES  # noqa: E402

SIM = os.path.join(ROOT, "tests", "sim", "libvvhip_sim.so")
pytestmark = pytest.mark.sim


def need():
    if not (os.path.exists(e2e_util.REF_HIP_SO) and os.path.exists(SIM)):
        pytest.skip("needs oracle/_ref/libvvenc_hip_enc.so and tests/sim/libvvhip_sim.so (python __graft_entry__.py)")
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present: the test double refuses to stand in for it")


def sim_env(**extra):
    e = {"LD_PRELOAD": SIM}
    e.update({k: str(v) for k, v in extra.items()})
    return e


CLIP = dict(w=208, h=120, in_bd=10, int_bd=10)


@pytest.mark.parametrize("preset", ["faster", "fast", "medium"])
def test_every_hook_every_preset(preset):
    """all tables + batched search sites + per-CTU ALF hooks, one encoder thread"""
    need()
    clip = dict(CLIP, frames=5, preset=preset)
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, mask=ALL_TABLES + BATCHED_SITES + 2048 + 4096 + 16384 + 32768), env=sim_env())
    assert hip["calls"][0] > 1000 and hip["calls"][10] > 50 and hip["calls"][12] > 50 and hip["calls"][14] >= 4, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


def test_every_hook_four_encoder_threads():
    """the reference's worker threads call the table entries and the per-CTU hooks concurrently: per-thread contexts and per-thread hook state, no host lock"""
    need()
    clip = dict(CLIP, frames=9, preset="faster", threads=4)
    cpu = run(dict(clip, hip=False, mask=0))
    for _ in range(2):
        hip = run(dict(clip, hip=True, mask=ALL_TABLES + BATCHED_SITES + 2048 + 4096 + 16384 + 32768), env=sim_env())
        assert hip["calls"][17] > 4 and hip["calls"][27] >= 2, hip["calls"]
        assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.parametrize("preset", ["faster", "medium"])
def test_simd_switch_selects_the_binding(preset):
    """--SIMD=HIP through vvenc_set_SIMD_extension: production set (MCTF search with all references of a picture in one device call + filter, whole-picture ALF statistics;
    whole-picture ALF filtering is bit-exact but not in the set: it loses at 8 encoder threads), 4 encoder threads -> several worker contexts"""
    need()
    clip = dict(CLIP, frames=17, preset=preset, threads=4)
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, simd="HIP"), env=sim_env())
    c = hip["calls"]
    assert c[9] >= 1 and c[16] >= 1 and c[19] == 0, c
    assert c[21] >= 1 and c[7] // 1000000 > c[21], c                   # fewer device ME calls than motion fields: references were batched
    assert c[27] >= 2 and c[28] == 1, c                                # worker contexts, one GPU
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


def test_alf_picture_statistics_follow_the_saturation_rule():
    """the whole-picture ALF statistics call sits in the serial filter derivation: the binding takes it only from $VVHIP_ALF_MIN_CTUS_PER_THREAD CTUs per encoder thread on
    (default 100: 1080p with <= 4 threads, 4K with <= 16); below it the per-CTU CPU tasks stay — same bitstream either way"""
    need()
    clip = dict(CLIP, frames=9, preset="faster", threads=4)
    cpu = run(dict(clip, hip=False, mask=0))
    off = run(dict(clip, hip=True, simd="HIP"), env=sim_env(VVHIP_ALF_MIN_CTUS_PER_THREAD=100))
    on = run(dict(clip, hip=True, simd="HIP"), env=sim_env(VVHIP_ALF_MIN_CTUS_PER_THREAD=1))
    assert off["calls"][16] == 0 and on["calls"][16] >= 1 and off["calls"][9] >= 1, (off["calls"], on["calls"])
    assert off["md5"] == cpu["md5"] and on["md5"] == cpu["md5"]


@pytest.mark.parametrize("clip", [dict(w=416, h=240, frames=9, preset="faster", threads=4),          # statistics units of 128 = two CTU rows of 64 (the last unit row: one)
                                  dict(w=208, h=120, frames=5, preset="medium", threads=2)])         # CTU 128 = unit
def test_alf_picture_statistics_in_bands(clip):
    """the statistics task of every CTU row reports to the binding (alfRow); a statistics-unit row whose CTU rows are all in goes to the device at once
    (upload of its rows + classification + statistics + download, asynchronously on the reporting worker's context), deriveFilter only collects.  Same stream as the CPU
    encoder's and as the whole-picture call's ($VVHIP_ALF_BANDS=0); every picture's statistics came from bands, one band per unit row"""
    need()
    clip = dict(clip, in_bd=10, int_bd=10)
    cpu = run(dict(clip, hip=False, mask=0))
    bands = run(dict(clip, hip=True, mask=8192), env=sim_env())
    whole = run(dict(clip, hip=True, mask=8192), env=sim_env(VVHIP_ALF_BANDS=0))
    cb, cw = bands["calls"], whole["calls"]
    unit = 128
    rows = (clip["h"] + unit - 1) // unit
    assert cb[16] >= 1 and cb[40] == cb[16] and cb[39] == rows * cb[16], cb
    assert cw[16] == cb[16] and cw[39] == 0 and cw[40] == 0, cw
    assert bands["md5"] == cpu["md5"] and whole["md5"] == cpu["md5"] and bands["bytes"] == cpu["bytes"], (cpu, bands, whole)


def test_residual_loop_batched_site():
    """hook bit 262144: the DCT-2 forward transforms of a CU's component TUs (InterSearch::xEstimateInterResidualQT) come from ONE device round trip per CU; TrQuant::xT finds
    them by content (a memo of a pure function), everything else of the loop runs as before"""
    need()
    clip = dict(CLIP, frames=9, preset="faster", threads=2)
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, mask=262144), env=sim_env())
    c = hip["calls"]
    assert c[31] > 50 and c[32] > c[31], c                              # CUs prefetched; transforms served from them (up to three per CU)
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


def test_merge_pruning_batched_site():
    """hook bit 524288: the SATD costs of a CU's regular merge candidates (EncCu::addRegularCandsToPruningList) come from ONE device call after the predictions are generated;
    the pruning list receives them in the original order"""
    need()
    clip = dict(CLIP, frames=9, preset="faster", threads=2)
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, mask=524288), env=sim_env())
    c = hip["calls"]
    assert c[34] > 50 and c[35] > c[34], c                              # CUs scored on the device; several candidates per call
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


def test_simd_switch_refuses_without_device():
    """no device library double, no GPU: --SIMD=HIP must fail loudly (the encoder reports the request as unsupported), never fall back silently"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so not built")
    if os.path.exists("/dev/kfd"):
        pytest.skip("GPU present")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import e2e_util as E; L = E.load(True); "
                        "yuv = E.synth_yuv(64, 64, 2, 8, 1); E.encode(L, yuv, 64, 64, 8, 8, simd='HIP')" % os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and ("no MI355X context" in r.stderr or "refused" in r.stderr), (r.returncode, r.stderr[-500:])


def test_pictures_shard_over_devices():
    """one picture <-> one device: two and four simulated devices, MCTF-filtered pictures and ALF pictures round-robin, originals needed on a second device are copied
    device-to-device; bitstream unchanged"""
    need()
    clip = dict(CLIP, frames=25, preset="medium", threads=4)
    cpu = run(dict(clip, hip=False, mask=0))
    for n in (2, 4):
        hip = run(dict(clip, hip=True, simd="HIP"), env=sim_env(VVHIP_SIM_DEVICES=n, VVHIP_GPUS="all"))
        c = hip["calls"]
        assert c[28] == n and c[27] >= n, c                            # GPUs in use, contexts on each
        assert c[24] >= 1, c                                           # device-to-device picture copies happened
        assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (n, cpu, hip)


def test_sharded_long_sequence_recycles_picture_buffers():
    """65 frames on three devices: the encoder recycles its original-picture buffers for later POCs, so resident mirrors are dropped and re-made while worker threads and the MCTF
    thread hold bindings to different devices (nested device scopes: ADVICE r2, GpuScope) — same bitstream, and every device served MCTF calls"""
    need()
    clip = dict(CLIP, frames=65, preset="faster", threads=4)
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, simd="HIP"), env=sim_env(VVHIP_SIM_DEVICES=3, VVHIP_GPUS="all"))
    c = hip["calls"]
    assert c[28] == 3 and c[21] >= 6 and c[22] > 16 * 3, c                 # three devices, MCTF device calls, more uploads than the resident capacity: buffers were recycled
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


def test_reference_pictures_resident_for_the_search_sites():
    """reconstructed pictures are mirrored CTU row by CTU row (EncSlice border extension); the TZ diamond rounds and the sub-pel refinement stages then address the reference
    picture in device memory (offsets only) instead of staging a window per call; two logical devices: every device gets every reconstruction"""
    need()
    clip = dict(CLIP, frames=9, preset="medium", threads=4)
    cpu = run(dict(clip, hip=False, mask=0))
    for env in (sim_env(), sim_env(VVHIP_LOGICAL_GPUS=2, VVHIP_GPUS=2)):
        hip = run(dict(clip, hip=True, mask=1 + 256 + 1024), env=env)
        c = hip["calls"]
        assert c[29] >= 9 and c[30] > 1000 and c[10] > 100 and c[12] > 100, c      # CTU-row uploads, search calls served from resident pictures
        assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


def test_lfnst_tus_stay_with_the_cpu_quantiser():
    need()
    clip = dict(CLIP, frames=5, preset="fast", options="RDOQ=0;DepQuant=0;LFNST=1")
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, mask=4), env=sim_env())
    assert hip["calls"][4] > 1000 and hip["calls"][20] == 0 and hip["calls"][38] > 100, hip["calls"]          # (round 6: LFNST TUs are quantised behind the C ABI too)
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


def test_shim_tables_against_the_double():
    """tests/cpp/test_shim (the C++ parity test of the table-shaped shim, a -m gpu test on a GPU box) against the test double: staging, registry and batching paths"""
    exe = os.path.join(ROOT, "tests", "cpp", "test_shim")
    if not (os.path.exists(exe) and os.path.exists(SIM)) or os.path.exists("/dev/kfd"):
        pytest.skip("tests/cpp/test_shim or the test double not built, or GPU present")
    e = dict(os.environ, LD_PRELOAD=SIM)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0 and "shim parity OK" in r.stdout, (r.stdout[-500:], r.stderr[-500:])


def test_mctf_stages_keep_the_default_stream_on_the_pan_clip():
    """round 6: on the 416x240 'pan' clip the reference's --SIMD=SCALAR stream differs from its default stream with MCTF on.  With the encoder's MCTF search (16), filter (128)
    and table entries (8) running on the test double — i.e. on the oracle's SCALAR-row arithmetic — the stream is still the DEFAULT one: whatever makes the reference's two
    rows disagree on this clip, it is not the arithmetic of the path this repository replaces."""
    need()
    clip = dict(w=416, h=240, frames=9, in_bd=10, int_bd=10, clip="pan", threads=4)
    default = run(dict(clip, hip=False, simd=None, mask=0))
    scalar = run(dict(clip, hip=False, simd="SCALAR", mask=0))
    for mask in (16, 128, 16 + 128, 8):
        sim = run(dict(clip, hip=True, mask=mask), env=sim_env())
        assert sim["md5"] == default["md5"], (mask, default, sim)
    assert scalar["md5"] != default["md5"] or True          # (reported, not required: the reference's own rows)
    print("default", default["md5"], "scalar", scalar["md5"])
