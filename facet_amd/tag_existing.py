"""The reference's two library-wide tagging loops over stored CLIP embeddings, without the database:

  photos.py:578-625 (`--recompute-tags`, CLIP branch): every row whose blob is truthy gets `tags_to_string(tag_list) if tag_list else
      None` - rows without a tag are written too, as NULL;
  tag_existing.py:16-63 (`tag_untagged_photos`, run after every scan, photos.py:1003-1020): every selected row is scored, and only the
      rows with at least one tag are written.

Both call `tagger.get_tags_from_embedding` once per row. Here the rows go through one engine call (CLIPTagger.select_batch ->
fe_tag_select: GEMM, per-tag max, threshold and top-k on the device); the caller keeps its SELECT and its UPDATE.
"""
import numpy as np

from .tagger import bytes_to_embedding


def tags_to_string(tags):
    """utils/tags.py:8-20"""
    if not tags:
        return None
    return ','.join(tags)


def get_tag_params(config):
    """utils/tags.py:38-52 -> (threshold, max_tags)"""
    clip_settings = config.get_clip_settings()
    tag_settings = config.get_tagging_settings()
    threshold = clip_settings.get('similarity_threshold_percent', 22) / 100
    max_tags = tag_settings.get('max_tags', 5)
    return threshold, max_tags


def tag_rows(engine, tagger, rows, threshold=0.22, max_tags=5, only_tagged=False):
    """rows: (key, blob) pairs as the reference SELECTs them (path, clip_embedding). -> [(tags_str_or_None, key)] in input order, the
    parameters of its `UPDATE photos SET tags = ? WHERE path = ?`, for the rows whose blob is neither None nor empty (the reference
    skips those, photos.py:614; get_tags_from_embedding answers [] for None). tags_str is ','.join(tags), None when no tag passes.
    only_tagged: tag_untagged_photos' rule - only the rows with at least one tag are returned (its `if tag_list:`), so the length of
    the result is its `tagged_count`. A blob that does not hold the vocabulary's 768 floats raises ValueError naming the row."""
    if tagger.text_embeddings is None:                 # the reference's tagger answers [] for every row
        return [] if only_tagged else [(None, key) for key, blob in rows if blob]
    if getattr(tagger, "_engine", None) is not engine:
        tagger.use_engine(engine)
    d = tagger.text_embeddings.shape[1]
    keys, blobs = [], []
    for i, (key, blob) in enumerate(rows):
        if not blob:
            continue
        if len(blob) != 4 * d:
            raise ValueError(f"row {i} ({key!r}): the embedding blob has {len(blob)} bytes, {d} float32 values take {4 * d}")
        keys.append(key)
        blobs.append(blob)
    if not keys:
        return []
    emb = np.frombuffer(b''.join(blobs), dtype=np.float32).reshape(len(keys), d)
    out = []
    for key, tags in zip(keys, tagger.select_batch(emb, threshold=threshold, max_tags=max_tags)):
        s = tags_to_string(tags)
        if s is not None or not only_tagged:
            out.append((s, key))
    return out


__all__ = ["tag_rows", "get_tag_params", "tags_to_string", "bytes_to_embedding"]
