"""End-to-end bit-exactness gate (BASELINE metric: "bit-exact vs CPU"): the REAL reference encoder, compiled from /root/reference into
oracle/_ref/, encodes a synthetic clip
  * with its scalar, SSE4.1 and AVX2 kernel rows (the reference's own invariant, cmake/modules/vvencTests.cmake:52-53)      [CPU tier]
  * with its kernel tables pointed at the HIP back-end through the table-shaped shim (build with the binding, bindings/vvenc/):
    RdCost distortion entries, fused 2-D transforms, Quant cores, MCTF error entries and the whole-picture MCTF ME          [GPU tier]
and every bitstream must have the same md5.  Each run is a separate process (the SIMD level is process-wide state in the reference)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the small test clips have a handful of CTUs per encoder thread: take the whole-picture ALF statistics hook regardless of the binding's saturation rule (vvenc_hip_binding.cpp: alfPictureOn)
os.environ.setdefault("VVHIP_ALF_MIN_CTUS_PER_THREAD", "0")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import e2e_util  # noqa: E402

WORKER = r'''
import sys, json
sys.path.insert(0, %r)
import e2e_util as E
cfg = json.loads(sys.argv[1])
L = E.load(cfg["hip"])
simd = cfg.get("simd")
if cfg["hip"] and not (simd or "").startswith("HIP"):
    assert L.vvref_install_hip_hooks(cfg["mask"]) == 0           # test entry; "simd": "HIP[:mask]" goes through the encoder's own --SIMD switch instead
if cfg.get("clip") == "pan":
    import e2e_fps as F
    yuv = F.synth_clip(cfg["w"], cfg["h"], cfg["frames"])
else:
    yuv = E.synth_yuv(cfg["w"], cfg["h"], cfg["frames"], cfg["in_bd"], 1234)
md5, n, secs = E.encode(L, yuv, cfg["w"], cfg["h"], cfg["in_bd"], cfg["int_bd"], preset=E.PRESETS[cfg.get("preset", "faster")], simd=simd, threads=cfg.get("threads", 1),
                        options=cfg.get("options"))
calls = None
if cfg["hip"]:
    import numpy as np
    c = np.zeros(43, np.uint64); L.vvref_hip_hook_calls_ex(c.ctypes.data, 43); calls = [int(x) for x in c]
print(json.dumps({"md5": md5, "bytes": n, "secs": secs, "calls": calls}))
''' % os.path.join(ROOT, "tests")


def run(cfg, timeout=1700, env=None):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", WORKER, json.dumps(cfg)], capture_output=True, text=True, timeout=timeout, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


CFG1 = dict(w=64, h=64, frames=8, in_bd=8, int_bd=8)          # BASELINE configs[0]
CFG10 = dict(w=128, h=64, frames=9, in_bd=10, int_bd=10)      # a 10-bit clip


@pytest.mark.ref
@pytest.mark.parametrize("clip", [CFG1, CFG10], ids=["cfg0-64x64-8b", "128x64-10b"])
def test_reference_rows_agree(clip):
    if not os.path.exists(e2e_util.REF_SO):
        pytest.skip("oracle/_ref not built")
    res = [run(dict(clip, hip=False, simd=s, mask=0)) for s in (None, "SCALAR", "SSE41")]
    assert len({r["md5"] for r in res}) == 1, res
    if os.path.exists(e2e_util.REF_HIP_SO):      # the hook-enabled build with hooks off is the reference
        assert run(dict(clip, hip=True, simd=None, mask=0))["md5"] == res[0]["md5"]


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [CFG1, CFG10], ids=["cfg0-64x64-8b", "128x64-10b"])
def test_hip_backend_bitstream_identical(clip):
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    cpu = run(dict(clip, hip=False, simd=None, mask=0))
    hip = run(dict(clip, hip=True, simd=None, mask=31))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][0] > 1000 and hip["calls"][2] > 10, hip["calls"]      # the encoder really went through the HIP entries
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"]


@pytest.mark.gpu
def test_hip_table_entries_only_bitstream_identical():
    """same gate with the MCTF search left to the reference's own schedule calling our per-candidate table entries
    (m_motionErrorLumaInt8 / m_motionErrorLumaFrac8[1] / m_calcVar through the shim) instead of the whole-picture device ME"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    cpu = run(dict(CFG1, hip=False, simd=None, mask=0))
    hip = run(dict(CFG1, hip=True, simd=None, mask=15))
    print("cpu", cpu, "hip", hip)
    assert 0 < hip["calls"][7] < 1000000, hip["calls"]
    assert hip["md5"] == cpu["md5"]


@pytest.mark.gpu
def test_hip_tcoeffops_slots_bitstream_identical():
    """the reference's global g_tCoeffOps pointed at the device slots (identical signatures, zero source change): every matrix-core
    pass, round/clip and Pel<->TCoeff copy of the encode runs on the GPU one call at a time; bitstream must not change"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    cpu = run(dict(CFG1, hip=False, simd=None, mask=0))
    hip = run(dict(CFG1, hip=True, simd=None, mask=32))
    print("cpu", cpu, "hip", hip)
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)
    assert hip["calls"][2] > 100 and hip["calls"][3] > 100, hip["calls"]


@pytest.mark.gpu
def test_hip_interpolation_tables_bitstream_identical():
    """every InterpolationFilter table slot of the encoder (m_filterHor/Ver, m_filterCopy, m_filter4x4/8xH/16xH) points at
    the device entries, so all motion compensation and sub-pel refinement planes of the encode are interpolated on the GPU (one call at a
    time); bitstream must not change"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    cpu = run(dict(CFG1, hip=False, simd=None, mask=0))
    hip = run(dict(CFG1, hip=True, simd=None, mask=64))
    print("cpu", cpu, "hip", hip)
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)
    assert hip["calls"][8] > 100, hip["calls"]


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [CFG1, CFG10], ids=["cfg0-64x64-8b", "128x64-10b"])
def test_hip_mctf_stage_on_device_bitstream_identical(clip):
    """the whole MCTF stage of the encoder on the GPU — hierarchical motion estimation (mask 16) AND the bilateral filter
    (mask 128) — against the CPU encode.  The device filter equals the reference's scalar row; its AVX2 row (the CPU run here) is allowed
    +-1 by the reference's unit test, and on these clips the bitstreams are identical."""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    cpu = run(dict(clip, hip=False, simd=None, mask=0))
    hip = run(dict(clip, hip=True, simd=None, mask=16 + 128))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][9] >= 1 and hip["calls"][7] >= 1000000, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.gpu
def test_hip_backend_multithreaded_encoder_bitstream_identical():
    """the encoder's own worker threads (4) call the table entries concurrently (RdCost/TrQuant/Quant are per worker, g_tCoeffOps and MCTF
    are shared: SURVEY 8b "Threading"); the shim serialises its staging area.  Every table on the device (mask 31 + interpolation 64 +
    MCTF filter 128), bitstream equal to the single-threaded CPU encode's (the reference's multi-threading is deterministic)."""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    cpu = run(dict(CFG10, hip=False, simd=None, mask=0, threads=4))
    hip = run(dict(CFG10, hip=True, simd=None, mask=31 + 64 + 128, threads=4))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][0] > 1000 and hip["calls"][8] > 100 and hip["calls"][9] >= 1, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [CFG1, CFG10], ids=["cfg0-64x64-8b", "128x64-10b"])
def test_hip_batched_subpel_refinement_bitstream_identical(clip):
    """the batching boundary at work inside the real encoder: every half- and quarter-sample stage of InterSearch::xPatternRefinement gets its
    (up to) nine candidate costs from ONE vvhip_subpel_refine_batch call (through vvhip::RdCost::patternRefineCosts); the encoder's own loop
    replays them (skip and break rules, MV-bit costs, strict < update, patternId bookkeeping).  Everything else on the CPU."""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    cpu = run(dict(clip, hip=False, simd=None, mask=0))
    hip = run(dict(clip, hip=True, simd=None, mask=256))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][10] > 50, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [CFG1, CFG10], ids=["cfg0-64x64-8b", "128x64-10b"])
def test_hip_dmvr_search_bitstream_identical(clip):
    """SURVEY 8f rank 3 against the real DMVR::xProcessDMVR: the refinement search of every sub-block of a CU comes from ONE
    vvhip_dmvr_refine_batch call (vvhip::DMVROps::refineCu); the encoder copies mvdL0SubPu / the BDOF switch from the results and does the final
    motion compensation itself.  DMVR is decoder-normative: any deviation changes the bitstream."""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    cpu = run(dict(clip, hip=False, simd=None, mask=0))
    hip = run(dict(clip, hip=True, simd=None, mask=512))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][11] > 10, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.gpu
def test_hip_alf_statistics_bitstream_identical():
    """SURVEY 8f rank 4 inside the real encoder: every CTU's ALF classification and covariance records (luma 7x7 x 25 classes, both chroma 5x5) come from the
    device (hook mask 2048, vvhip::ALFOps) instead of deriveClassification / getPreBlkStats.  The ALF filter derivation works on these floats — a single
    differently rounded sum can change a coefficient — so identical bitstreams pin the float accumulation order in the real pipeline."""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=208, h=120, frames=9, in_bd=10, int_bd=10, threads=2)
    cpu = run(dict(clip, hip=False, simd=None, mask=0))
    hip = run(dict(clip, hip=True, simd=None, mask=2048 + 4096))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][14] > 4 and hip["calls"][15] > 4, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.gpu
def test_hip_alf_picture_statistics_bitstream_identical():
    """the whole-picture form (hook mask 8192): the per-CTU statistics tasks of the encoder do nothing, EncAdaptiveLoopFilter::deriveFilter starts with ONE device
    call per picture (classification + luma / chroma records of every 128x128 statistics unit, CTU-by-CTU chains inside a unit); small clip and 1080p"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=208, h=120, frames=9, in_bd=10, int_bd=10, threads=2)
    cpu = run(dict(clip, hip=False, simd=None, mask=0))
    hip = run(dict(clip, hip=True, simd=None, mask=8192))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][16] >= 1, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)
    import e2e_fps
    res = [e2e_fps.run(dict(w=1920, h=1080, frames=9, threads=8, mask=m)) for m in (0, 8192)]
    print(res)
    assert res[1]["calls"][16] >= 1, res[1]["calls"]
    assert res[0]["md5"] == res[1]["md5"] and res[0]["bytes"] == res[1]["bytes"], res


@pytest.mark.gpu
def test_hip_alf_statistics_1080p_bitstream_identical():
    """the same at 1080p (preset faster: 64x64 CTUs inside 128x128 statistics units, so the float chains continue from CTU to CTU through the
    start records): 510 CTUs per ALF picture, 8 encoder threads"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    import e2e_fps
    res = [e2e_fps.run(dict(w=1920, h=1080, frames=9, threads=8, mask=m)) for m in (0, 2048 + 4096)]
    print(res)
    assert res[1]["calls"][14] >= 510 and res[1]["calls"][15] >= 510, res[1]["calls"]
    assert res[0]["md5"] == res[1]["md5"] and res[0]["bytes"] == res[1]["bytes"], res


@pytest.mark.gpu
def test_hip_alf_filtering_bitstream_identical():
    """ALF apply side inside the real encoder (hook masks 16384 + 32768): every CTU block that EncAdaptiveLoopFilter::reconstructCTU hands to m_filter7x7Blk / m_filter5x5Blk
    and applyCcAlfFilterCTU hands to m_filterCcAlf is filtered on the device instead.  The filtered reconstruction is the reference of the following pictures, so one
    differing sample changes the bitstream.  Small clip, and 1080p with the statistics on the device as well (8 encoder threads)."""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=208, h=120, frames=9, in_bd=10, int_bd=10, threads=2)
    cpu = run(dict(clip, hip=False, simd=None, mask=0))
    hip = run(dict(clip, hip=True, simd=None, mask=16384 + 32768))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][17] > 4, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)
    import e2e_fps
    res = [e2e_fps.run(dict(w=1920, h=1080, frames=9, threads=8, mask=m)) for m in (0, 8192 + 16384 + 32768)]
    print(res)
    assert res[1]["calls"][17] >= 500, res[1]["calls"]
    assert res[0]["md5"] == res[1]["md5"] and res[0]["bytes"] == res[1]["bytes"], res


@pytest.mark.gpu
def test_hip_alf_picture_filtering_bitstream_identical():
    """the whole ALF stage of a picture in two shim calls (hook masks 8192 + 65536): statistics of every unit before the derivation, and after it the filtering of every
    enabled CTU of the three planes by the first reconstruction task of the picture (the other tasks find the picture done); CC-ALF per block (32768)"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=208, h=120, frames=9, in_bd=10, int_bd=10, threads=2)
    cpu = run(dict(clip, hip=False, simd=None, mask=0))
    hip = run(dict(clip, hip=True, simd=None, mask=8192 + 65536))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][19] >= 1 and hip["calls"][17] == 0, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)
    import e2e_fps
    res = [e2e_fps.run(dict(w=1920, h=1080, frames=9, threads=8, mask=m)) for m in (0, 8192 + 65536 + 32768)]
    print(res)
    assert res[1]["calls"][19] >= 2 and res[1]["calls"][17] == 0, res[1]["calls"]
    assert res[0]["md5"] == res[1]["md5"] and res[0]["bytes"] == res[1]["bytes"], res


@pytest.mark.gpu
def test_hip_4k_picture_level_stages_bitstream_identical():
    """BASELINE's 4K geometry (3840x2160 10-bit, preset faster) in the real encoder: the picture-level stages on the device — MCTF search + bilateral filter (144), ALF
    statistics (8192) and ALF filtering (65536) of whole pictures — 9 frames, 8 encoder threads"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    import e2e_fps
    res = [e2e_fps.run(dict(w=3840, h=2160, frames=9, threads=8, mask=m)) for m in (0, 144 + 8192 + 65536)]
    print(res)
    assert res[1]["calls"][9] >= 1 and res[1]["calls"][16] >= 1 and res[1]["calls"][19] >= 1, res[1]["calls"]
    assert res[0]["md5"] == res[1]["md5"] and res[0]["bytes"] == res[1]["bytes"], res


@pytest.mark.gpu
def test_hip_everything_on_device_bitstream_identical():
    """all hooks at once on a larger clip (208x120 10-bit, 9 frames, 2 encoder threads): every kernel table, the interpolation tables, whole-picture
    MCTF ME + filter, batched integer diamond rounds, batched sub-pel refinement stages, per-CU DMVR searches, per-CTU ALF statistics and ALF / CC-ALF filtering"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=208, h=120, frames=9, in_bd=10, int_bd=10, threads=2)
    cpu = run(dict(clip, hip=False, simd=None, mask=0))
    hip = run(dict(clip, hip=True, simd=None, mask=31 + 64 + 128 + 256 + 512 + 1024 + 2048 + 4096 + 16384 + 32768))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][0] > 1000 and hip["calls"][8] > 100 and hip["calls"][9] >= 1 and hip["calls"][10] > 50 and hip["calls"][11] > 5 and hip["calls"][12] > 50 and hip["calls"][14] > 4, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [CFG1, CFG10], ids=["cfg0-64x64-8b", "128x64-10b"])
def test_hip_batched_tz_diamond_rounds_bitstream_identical(clip):
    """integer motion search through the batching boundary: when a TZ diamond round starts (InterSearch::xTZ8PointDiamondSearch) all positions it
    may test are scored by ONE device call (vvhip::RdCost::distAtPositions -> vvhip_dist_batch); xTZSearchHelp takes its SAD from that table and
    runs its own update logic (MV-bit cost, strict <).  Everything else on the CPU."""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    cpu = run(dict(clip, hip=False, simd=None, mask=0))
    hip = run(dict(clip, hip=True, simd=None, mask=1024))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][12] > 50 and hip["calls"][13] > hip["calls"][12], hip["calls"]      # rounds, looked-up positions
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# presets fast and medium (BASELINE configs[3..4] geometry: CTU 128 + MTT => rectangular CUs, GEO, SMVD, affine, LFNST, DepQuant, two references per list;
# source/Lib/vvenc/vvencCfg.cpp:2751-2893) through the same gates, on a 10-bit clip large enough for CTU 128 + MTT.  Four encoder threads: the table entries
# are called concurrently through per-thread device contexts.
CLIP416 = dict(w=416, h=240, in_bd=10, int_bd=10, threads=4)
ALL_TABLES = 31 + 64 + 128            # every kernel table, whole-picture MCTF search + filter
BATCHED_SITES = 1024 + 256 + 512      # TZ diamond rounds, sub-pel refinement stages, DMVR per CU
PICTURE_STAGES = 16 + 128 + 8192 + 65536


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["faster", "fast", "medium"])
def test_hip_presets_all_tables_bitstream_identical(preset):
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(CLIP416, frames=5, preset=preset)
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, mask=ALL_TABLES))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][0] > 10000 and hip["calls"][2] > 1000 and hip["calls"][8] > 1000, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["faster", "fast", "medium"])
def test_hip_presets_batched_search_sites_bitstream_identical(preset):
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(CLIP416, frames=5, preset=preset)
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, mask=BATCHED_SITES))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][10] > 100 and hip["calls"][12] > 100, hip["calls"]
    assert hip["calls"][29] >= 5 and hip["calls"][30] > 100, hip["calls"]      # reconstruction rows mirrored, search stages served from the resident reference pictures
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["faster", "fast", "medium"])
def test_hip_presets_picture_stages_through_simd_switch_bitstream_identical(preset):
    """the production selection, --SIMD=HIP (vvenc_set_SIMD_extension("HIP") -> VVEncImpl::setSIMDExtension -> vvenc_hip_select): MCTF search + filter and ALF statistics of
    whole pictures on the device (whole-picture ALF filtering is an explicit mask: it loses at 8 encoder threads); 17 frames so that MCTF filters two pictures"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(CLIP416, frames=17, preset=preset)
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, simd="HIP"))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][9] >= 1 and hip["calls"][21] >= 1 and hip["calls"][16] >= 1 and hip["calls"][19] == 0, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)
    full = run(dict(clip, hip=True, simd="HIP:%d" % PICTURE_STAGES))          # + whole-picture ALF filtering
    assert full["calls"][19] >= 1 and full["md5"] == cpu["md5"], (cpu, full)


@pytest.mark.gpu
@pytest.mark.parametrize("site,first,second", [(262144, 31, 32), (524288, 34, 35)], ids=["residual-loop", "merge-pruning"])
def test_hip_cu_level_sites_bitstream_identical(site, first, second):
    """the two CU-level call sites of SURVEY 8a outside the motion search: InterSearch::xEstimateInterResidualQT (a CU's component TUs forward-transformed in one device round
    trip, hook bit 262144) and EncCu::addRegularCandsToPruningList (a CU's regular merge candidates scored in one device call, bit 524288), on the 'pan' clip, 4 threads"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=416, h=240, frames=9, in_bd=10, int_bd=10, clip="pan", threads=4)
    cpu = run(dict(clip, hip=False, simd=None, mask=0))
    hip = run(dict(clip, hip=True, simd=None, mask=site))
    print(cpu, hip)
    assert hip["calls"][first] > 200 and hip["calls"][second] > hip["calls"][first], hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"]


@pytest.mark.gpu
def test_production_mask_equals_the_x86_row_where_the_references_rows_differ():
    """on the 416x240 'pan' clip the reference's OWN --SIMD=SCALAR stream differs from its default (AVX2) stream with MCTF on (equal with MCTF=0;BIM=0).
    north_star's comparison target is the x86 row: --SIMD=HIP (production mask: MCTF search + filter + ALF statistics on the device) must equal the DEFAULT stream there, and so
    must the MCTF stages alone (16 + 128).  The scalar stream is encoded next to them: this test fails if the device side ever follows it instead (or if either choice changes
    silently).  What the row difference is NOT (round 6, CPU tier): the MCTF search and filter — with both replaced by scalar-row arithmetic the encoder still emits the AVX2
    stream (tests/test_binding_sim.py::test_mctf_stages_keep_the_default_stream_on_the_pan_clip), and the filter's two rows agree sample for sample (tolerance 0)."""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=416, h=240, frames=9, in_bd=10, int_bd=10, clip="pan", threads=4)
    default = run(dict(clip, hip=False, simd=None, mask=0))
    scalar = run(dict(clip, hip=False, simd="SCALAR", mask=0))
    hip = run(dict(clip, hip=True, simd="HIP"))
    stages = run(dict(clip, hip=True, simd=None, mask=16 + 128))
    print("default", default["md5"], "scalar", scalar["md5"], "hip", hip["md5"], "mctf stages", stages["md5"])
    assert hip["calls"][21] >= 1 and hip["calls"][9] >= 1, hip["calls"]                      # the MCTF search and the filter really ran on the device
    assert stages["calls"][21] >= 1 and stages["calls"][9] >= 1, stages["calls"]
    assert hip["md5"] == default["md5"] and hip["bytes"] == default["bytes"], (default, hip)
    assert stages["md5"] == default["md5"], (default, stages)
    if scalar["md5"] != default["md5"]:
        assert hip["md5"] != scalar["md5"]                                                   # (documented: the device side is the x86 row's twin, not the scalar row's)
    off = "MCTF=0;BIM=0"
    three = [run(dict(clip, hip=h, simd=sd, mask=0, options=off))["md5"] for h, sd in ((False, "SCALAR"), (False, None), (True, "HIP"))]
    assert len(set(three)) == 1, three


@pytest.mark.gpu
def test_hip_lfnst_quantiser_guard_bitstream_identical():
    """ADVICE r1 / VERDICT r5 #8: with RDOQ and DepQuant off the encoder's scalar quantiser (Quant::xQuant) is the main path, and LFNST TUs must see QuantCore's
    first-coefficient-group rule (Quant.cpp:149-159).  Round 6: the rule is on the device (vvhip_quant_core_lfnst) — no TU is left to the CPU entry any more (counter 20 == 0,
    counter 38 counts the LFNST TUs the device quantised); $VVHIP_LFNST_QUANT_ON_CPU=1 is the old route and gives the same stream"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=208, h=120, frames=5, in_bd=10, int_bd=10, preset="fast", options="RDOQ=0;DepQuant=0;LFNST=1")
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, mask=4))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][4] > 1000 and hip["calls"][20] == 0 and hip["calls"][38] > 100, hip["calls"]      # device quantiser calls; no LFNST TU left to the CPU; LFNST TUs on the device
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)
    old = run(dict(clip, hip=True, mask=4), env={"VVHIP_LFNST_QUANT_ON_CPU": "1"})
    assert old["calls"][20] > 100 and old["calls"][38] == 0 and old["md5"] == cpu["md5"], (cpu, old)


@pytest.mark.gpu
def test_hip_4k_medium_picture_stages_bitstream_identical():
    """BASELINE configs[3] geometry: 3840x2160 10-bit, preset medium (CTU 128, MTT), picture-level stages on the device through --SIMD=HIP, 9 frames, 8 threads"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=3840, h=2160, frames=9, in_bd=10, int_bd=10, threads=8, preset="medium", clip="pan")
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, simd="HIP:73872"))          # production set + whole-picture ALF filtering (65536)
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][9] >= 1 and hip["calls"][16] >= 1 and hip["calls"][19] >= 1, hip["calls"]
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.gpu
def test_hip_8k_fast_picture_stages_bitstream_identical():
    """BASELINE configs[4] geometry: 7680x4320 10-bit, preset fast, picture-level stages on the device, 17 frames (two MCTF-filtered pictures: the temporal filter runs at 8K inside
    the encoder — calls[9]: MCTF filter pictures, [21]: device motion-estimation calls, [16] / [19]: ALF statistics / filter pictures), 8 threads (the ALF picture stages go
    to the device only while the thread pool is saturated)"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=7680, h=4320, frames=17, in_bd=10, int_bd=10, threads=8, preset="fast", clip="pan")
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, simd="HIP:73872"))
    print("cpu", cpu, "hip", hip)
    assert hip["calls"][9] >= 2 and hip["calls"][21] >= 2 and hip["calls"][16] >= 1 and hip["calls"][19] >= 1, hip["calls"]          # MCTF motion estimation + filter at 8K did run on the device
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.gpu
def test_hip_pictures_shard_over_logical_devices_bitstream_identical():
    """SURVEY 8e in the binding, on one physical GPU: VVHIP_LOGICAL_GPUS=2 makes the shim present two devices (both on GPU 0), VVHIP_GPUS=2 makes the binding spread the
    pictures over them — per-device registries, thread -> device binding per picture, device-to-device copies (hipMemcpyPeerAsync) of originals another device already holds.
    Preset medium (overlapping MCTF windows => peer copies), 25 frames, 4 threads; bitstream equal to the CPU encode's"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(CLIP416, frames=25, preset="medium")
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, simd="HIP"), env={"VVHIP_LOGICAL_GPUS": "2", "VVHIP_GPUS": "2"})
    print("cpu", cpu, "hip", hip)
    c = hip["calls"]
    assert c[28] == 2 and c[24] >= 1 and c[9] >= 1, c          # two devices in use, device-to-device picture copies, MCTF filter pictures
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


# ---- BASELINE configs at FULL length
@pytest.mark.gpu
def test_config2_4k_65_frames_faster_production_bitstream_identical():
    """BASELINE configs[2]: 3840x2160 10-bit, 65 frames, preset faster, --SIMD=HIP (MCTF block matching + filter and whole-picture ALF statistics on the MI355X), 8 encoder
    threads: the bitstream of the whole sequence equals the CPU encoder's"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    import e2e_fps
    cpu = e2e_fps.run(dict(w=3840, h=2160, frames=65, threads=8, mask=0), timeout=1200)
    hip = e2e_fps.run(dict(w=3840, h=2160, frames=65, threads=8, mask=16 + 128 + 8192), timeout=1200)
    print(cpu, hip)
    assert hip["calls"][9] >= 8 and hip["calls"][16] >= 8 and hip["calls"][21] >= 8, hip["calls"]      # MCTF-filtered pictures, ALF statistics pictures (ALF is off on the upper temporal layers), device ME calls
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.gpu
def test_config3_4k_medium_65_frames_two_logical_devices_bitstream_identical():
    """BASELINE configs[3] geometry over two GOPs + 1: 3840x2160 10-bit, 65 frames, preset medium (CTU 128, MTT), pictures sharded over two logical devices (one physical GPU:
    per-device registries, thread -> device binding, device-to-device picture copies), --SIMD=HIP, 8 threads"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=3840, h=2160, frames=65, in_bd=10, int_bd=10, threads=8, preset="medium", clip="pan")
    cpu = run(dict(clip, hip=False, mask=0))
    hip = run(dict(clip, hip=True, simd="HIP"), env={"VVHIP_LOGICAL_GPUS": "2", "VVHIP_GPUS": "2"})
    print("cpu", cpu, "hip", hip)
    c = hip["calls"]
    assert c[28] == 2 and c[9] >= 8 and c[16] >= 8, c
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


# ---- BASELINE configs[3] / [4] at FULL length: opt-in — `pytest -m "gpu and long"` (or VVHIP_LONG_TESTS=1); minutes of encoder time each, not part of the
#      default GPU suite.  The builder's runs of both are in profiles/r05_long_gates.log
@pytest.mark.gpu
@pytest.mark.long
def test_config3_4k_medium_129_frames_full_length_production_bitstream_identical():
    """BASELINE configs[3] at full length: 3840x2160 10-bit, 129 frames (four GOPs of 32 + 1), preset medium (CTU 128, MTT depth 1 / 2, GEO: vvencCfg.cpp:2821-2893),
    production mask through --SIMD=HIP, pictures sharded over two logical devices, 8 encoder threads: md5 == the CPU encoder's; MCTF and ALF device calls asserted.
    (8 threads: above that the encoder switches its inter-frame line synchronisation on (m_ifpLines > 0) and the binding leaves the whole-picture ALF statistics to the CPU tasks
    by design, bindings/vvenc/apply_binding.py; the 16-thread run of the same clip — md5 equal, 6.69 -> 7.08 fps — is in profiles/r05_long_gates.log)"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=3840, h=2160, frames=129, in_bd=10, int_bd=10, threads=8, preset="medium", clip="pan")
    cpu = run(dict(clip, hip=False, mask=0), timeout=3000)
    hip = run(dict(clip, hip=True, simd="HIP"), env={"VVHIP_LOGICAL_GPUS": "2", "VVHIP_GPUS": "2"}, timeout=3000)
    print("cpu", cpu, "hip", hip, "fps cpu %.2f hip %.2f" % (129 / cpu["secs"], 129 / hip["secs"]))
    c = hip["calls"]
    assert c[28] == 2 and c[9] >= 16 and c[21] >= 16 and c[16] >= 16, c          # two devices; MCTF-filtered pictures, device motion-estimation calls, ALF statistics pictures
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)


@pytest.mark.gpu
@pytest.mark.long
def test_config4_8k_fast_65_frames_full_length_production_bitstream_identical():
    """BASELINE configs[4] at full length: 7680x4320 10-bit, 65 frames, preset fast, production mask through --SIMD=HIP, 8 encoder threads: md5 == the CPU encoder's; the
    temporal filter's block matching and the ALF statistics ran on the device at 8K (16 threads, md5 equal, 3.44 -> 3.54 fps: profiles/r05_long_gates.log)"""
    if not os.path.exists(e2e_util.REF_HIP_SO):
        pytest.skip("oracle/_ref/libvvenc_hip_enc.so (the encoder with the binding) not built")
    clip = dict(w=7680, h=4320, frames=65, in_bd=10, int_bd=10, threads=8, preset="fast", clip="pan")
    cpu = run(dict(clip, hip=False, mask=0), timeout=3000)
    hip = run(dict(clip, hip=True, simd="HIP"), timeout=3000)
    print("cpu", cpu, "hip", hip, "fps cpu %.2f hip %.2f" % (65 / cpu["secs"], 65 / hip["secs"]))
    c = hip["calls"]
    assert c[9] >= 8 and c[21] >= 8 and c[16] >= 8, c
    assert hip["md5"] == cpu["md5"] and hip["bytes"] == cpu["bytes"], (cpu, hip)
