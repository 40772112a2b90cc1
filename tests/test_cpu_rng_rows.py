"""Specification of the sample-keyed keep-mask generator (oracle.rng.keep_mask_rows) and of the (outer, B, inner) triples
masks.MaskSet.draw hands to mstts_philox_keep_mask_rows.  tests/test_gpu_glue_ops.py compares the HIP kernel with keep_mask_rows bit for
bit; the identities here tie keep_mask_rows itself to the flat generator (keep_mask) and to its own sharding contract, so that
comparison has a checked reference.  Nothing here loads the HIP library."""
import numpy as np
import pytest

from multi_speaker_tts_amd import lib, masks
from multi_speaker_tts_amd.params import Dims
from oracle import model as OM, rng as orng, train as OT

SEED = 2 ** 40 + 17          # nonzero high key word


def test_one_sample_is_the_flat_generator():
    """B = 1, sample0 = 0: counter word 1 is 0 for every block, which is the flat generator's counter while n < 2^34 - on both axes."""
    flat = orng.keep_mask((1, 7, 9), SEED, 31, 0.9)
    assert 0 < int(flat.sum()) < flat.size
    assert np.array_equal(orng.keep_mask_rows((1, 7, 9), 0, SEED, 31, 0, 0.9), flat)
    assert np.array_equal(orng.keep_mask_rows((7, 1, 9), 1, SEED, 31, 0, 0.9), orng.keep_mask((7, 1, 9), SEED, 31, 0.9))


def test_a_sample_keeps_its_mask_under_sharding():
    """[5, 6, 10] step-major over 6 samples = the 2-sample shard at sample0 = 0 next to the 4-sample shard at sample0 = 2 (inner = 10: a
    four-draw block straddles two steps); the batch-major form shards along axis 0 the same way."""
    whole = orng.keep_mask_rows((5, 6, 10), 1, SEED, 12, 0, 0.9)
    assert np.array_equal(whole[:, :2], orng.keep_mask_rows((5, 2, 10), 1, SEED, 12, 0, 0.9))
    assert np.array_equal(whole[:, 2:], orng.keep_mask_rows((5, 4, 10), 1, SEED, 12, 2, 0.9))
    assert not np.array_equal(whole[:, 2:], orng.keep_mask_rows((5, 4, 10), 1, SEED, 12, 0, 0.9))      # the offset matters
    whole0 = orng.keep_mask_rows((6, 5, 10), 0, SEED, 12, 0, 0.9)
    assert np.array_equal(whole0[2:], orng.keep_mask_rows((4, 5, 10), 0, SEED, 12, 2, 0.9))
    assert np.array_equal(whole0, whole.transpose(1, 0, 2))                                              # one sample, one mask, either layout


def test_sample_counter_wraps_at_32_bits():
    """The sample index is a 32-bit counter word: samples 2 and 3 of a draw at sample0 = 2^32 - 2 are global samples 0 and 1."""
    hi = orng.keep_mask_rows((3, 4, 5), 1, SEED, 30, 2 ** 32 - 2, 0.5)
    lo = orng.keep_mask_rows((3, 2, 5), 1, SEED, 30, 0, 0.5)
    assert np.array_equal(hi[:, 2:], lo)
    assert not np.array_equal(hi[:, :2], lo)


@pytest.mark.parametrize("rank", [0, 3])
def test_maskset_draw_arguments(monkeypatch, rank):
    """Every mask of a training-shape table (vocoder and speaker stack included): draw passes (outer, B, inner) = (1, B, T * C) for the
    batch-major conv-block dropouts and (S, B, C) for the step-major rest, sample0 = rank * B, the table's stream and keep probability -
    the same triple oracle.rng.keep_mask_rows derives from (shape, batch axis).  The entry point is replaced by a recorder: no library."""
    d, od = Dims(), OM.Dims()
    B, T_enc, S, W = 32, 160, 801, 32 * d.spk_samples
    calls, loaded = [], lib._lib
    monkeypatch.setattr(lib, "call", lambda name, *a: calls.append((name,) + a))
    ms = masks.MaskSet(d, B, T_enc, S, True, device=None, rank=rank, alloc=lambda n: None, vocoder=True, speaker_windows=W)
    ms.draw(SEED)
    spec = masks.table(d, B, T_enc, S, True, speaker_windows=W, vocoder=True)
    assert spec == OT.mask_table(od, B, T_enc, S, True, speaker_windows=W, vocoder=True)
    assert len(calls) == len(spec) and len({s[0] for s in spec}) == len(spec) and len({s[1] for s in spec}) == len(spec)
    seen = set()
    for (name, stream, shape, keep), c in zip(spec, calls):
        assert len(shape) == 3 and masks.batch_axis(name) == OT.mask_batch_axis(name)
        if name.startswith(("enc_conv_drop", "post_drop")):
            assert masks.batch_axis(name) == 0 and shape[0] == B
            want = (1, B, shape[1] * shape[2])
        else:
            assert masks.batch_axis(name) == 1
            nb = W if name.startswith("s_z") else B
            assert shape[1] == nb
            want = (shape[0], nb, shape[2])
        assert c[0] == "mstts_philox_keep_mask_rows" and c[1] is None
        assert tuple(c[2:5]) == want, name
        assert c[5] == SEED and c[6] == stream and c[7] == rank * want[1] and c[8] == pytest.approx(keep)
        seen.add(name.rstrip("0123456789"))
    assert seen == {"prenet_drop_", "enc_conv_drop_", "enc_zc_fw", "enc_zh_fw", "enc_zc_bw", "enc_zh_bw", "dec_zc_", "dec_zh_", "post_drop_",
                    "v_zc_fw", "v_zh_fw", "v_zc_bw", "v_zh_bw", "s_zc_", "s_zh_"}
    assert lib._lib is loaded          # the recorder stood in for the library: nothing above loaded it
