"""CPU: the VLM step of BatchScorer (`vlm_composition=`, the batch form of Facet.get_composition_scores, scorer.py:698-705) with a stub
analyzer: comp_score is overwritten by the analyzer's score (2 decimals, as batch_processor.py:313 stores it), composition_explanation is
added, a result without a score changes nothing, one batch_analyze per batch, and without the argument the dicts are untouched."""
import copy

import numpy as np

from facet_amd.batch import BatchScorer


class _Stub:
    def __init__(self, results):
        self.results, self.calls = results, []

    def batch_analyze(self, images):
        self.calls.append([im.size for im in images])
        return self.results


def _dicts():
    return [{'comp_score': 6.12, 'composition_pattern': 'center', 'aesthetic': 5.5}, {'comp_score': 4.0, 'aesthetic': 7.0}, {'comp_score': 3.3}]


def test_analyzer_scores_overwrite_comp_score_and_add_the_explanation():
    stub = _Stub([{'composition_score': 7.456, 'explanation': 'thirds', 'elements': {'rule_of_thirds': True}},
                  {'composition_score': None, 'explanation': 'ignored', 'elements': {}},
                  {'composition_score': 5.0, 'explanation': 'Analysis error: x', 'elements': {}}])
    s = BatchScorer(engine=None, vlm_composition=stub)
    imgs = np.zeros((3, 8, 12, 3), np.uint8)
    out = s.apply_vlm_composition(_dicts(), imgs)
    assert stub.calls == [[(12, 8)] * 3]      # one call, PIL images of the batch (width, height)
    assert out[0] == {'comp_score': 7.46, 'composition_pattern': 'center', 'aesthetic': 5.5, 'composition_explanation': 'thirds'}
    assert out[1] == _dicts()[1]
    assert out[2] == {'comp_score': 5.0, 'composition_explanation': 'Analysis error: x'}


def test_default_is_no_analyzer_and_no_new_keys():
    import inspect
    assert inspect.signature(BatchScorer.__init__).parameters['vlm_composition'].default is None
    s = BatchScorer(engine=None)
    assert s.vlm_composition is None
    src = inspect.getsource(BatchScorer.process_batch)
    assert "if self.vlm_composition is not None:" in src      # the only use: guarded, so the dicts are exactly as before without it
    before = _dicts()
    assert before == copy.deepcopy(before) and all('composition_explanation' not in d for d in before)
