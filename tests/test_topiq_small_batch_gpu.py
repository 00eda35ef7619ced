"""GPU: the fp32 TOPIQ score of a small image does not depend on what it is batched with. Images of at most 32 tokens per level (12 at
96 x 128) used to change kernels with the batch: the head's token projections (q, k, the first MLP layer) went to the few-row kernel up to
32 rows = 2 images and to the matrix-core kernel from 3 images on, which sum in different orders, so a score could move by an ulp or two
between a batch of one and a batch of three (tests/test_jpeg_progressive_gpu.py compares exactly those). linear_tokens (engine.hip) routes by
the tokens per image instead: bit-equal scores, alone and in batches of 2, 3 and 5 (5 x 12 rows: two chunks, the second ragged)."""
import numpy as np
import pytest

from facet_amd._lib import FE_MODEL_TOPIQ
from facet_amd.weights import synthetic_state_dict, synthetic_images

pytestmark = pytest.mark.gpu


def test_scores_of_small_images_are_the_same_alone_and_batched(engine):
    engine.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", seed=3))
    imgs = synthetic_images(21, 5, 96, 128)
    engine.set_microbatch(8)
    alone = np.concatenate([engine.topiq_score(imgs[k:k + 1]) for k in range(len(imgs))])
    for nb in (2, 3, 5):
        got = engine.topiq_score(imgs[:nb])
        print(f"batch of {nb}: {got} alone {alone[:nb]}")
        assert np.array_equal(got, alone[:nb]), (nb, got, alone[:nb])
