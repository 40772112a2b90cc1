"""The six forms the GEMM entry points are tested in (tests/test_gpu_conv_window_ref.py, tests/test_gpu_gemm_plain_ref.py): which process-wide
scheduling switches a form sets, and the context manager that sets them and puts the defaults back.
    f32_mfma     mstts_gemm_f32 after mstts_gemm_split3(0): v_mfma_f32_32x32x2_f32 for everything
    split_128    split3 with mstts_gemm_split_big(0): gemm_split_kernel wherever its conditions hold
    split_big    split3, big tiles and mstts_gemm_big_min_workgroups(1, 1): gemm_split_big_kernel wherever M, N >= 192
    default_det  the defaults under lib.deterministic_gemm(): no K-cut of the library's own
    bf16_128     mstts_gemm_bf16 after mstts_gemm_bf16_big(0)
    bf16_big     mstts_gemm_bf16 with big tiles and the minimum lowered: gemm_bf16_big_kernel wherever M, N >= 192"""
import contextlib

# split3, split_big, bf16_big, lowered minimums, deterministic, entry point
FORMS = {
    "f32_mfma": dict(split3=0, split_big=1, bf16_big=1, low_min=False, det=False, bf16=False),
    "split_128": dict(split3=1, split_big=0, bf16_big=1, low_min=False, det=False, bf16=False),
    "split_big": dict(split3=1, split_big=1, bf16_big=1, low_min=True, det=False, bf16=False),
    "default_det": dict(split3=1, split_big=1, bf16_big=1, low_min=False, det=True, bf16=False),
    "bf16_128": dict(split3=1, split_big=1, bf16_big=0, low_min=False, det=False, bf16=True),
    "bf16_big": dict(split3=1, split_big=1, bf16_big=1, low_min=True, det=False, bf16=True),
}


def _defaults(L):
    L.mstts_gemm_split3(1)
    L.mstts_gemm_split_big(1)
    L.mstts_gemm_bf16_big(1)
    L.mstts_gemm_big_min_workgroups(160, 160)
    L.mstts_gemm_deterministic(0)


@contextlib.contextmanager
def _form(form):
    from multi_speaker_tts_amd import lib
    f, L = FORMS[form], lib.load()
    try:
        L.mstts_gemm_split3(f["split3"])
        L.mstts_gemm_split_big(f["split_big"])
        L.mstts_gemm_bf16_big(f["bf16_big"])
        if f["low_min"]:
            L.mstts_gemm_big_min_workgroups(1, 1)
        with (lib.deterministic_gemm() if f["det"] else contextlib.nullcontext()):
            yield f
    finally:
        _defaults(L)
