"""Drop-in for reference models/tagger.py `CLIPTagger` (tag selection from a stored 768-d embedding).

Same interface (:20-158): CLIPTagger(clip_model, device, config); get_tags_from_embedding(bytes, threshold, max_tags);
get_tags_with_scores; is_artwork; attrs tag_vocabulary, text_embeddings. The text tower is not in the engine yet
(SURVEY §8f-3), so text embeddings come either from `clip_model.encode_text` when the given model has one, or from
`set_text_embeddings()` (precomputed [T,768], L2-normalised). Without them every call returns [] exactly like the
reference does when `clip_model is None` (:38-39, :89-90).

Whole libraries: `use_engine(engine)` hands the vocabulary to the engine once, and `select_batch` / `scores_batch` / `is_artwork_batch`
answer get_tags_from_embedding / get_tags_with_scores / is_artwork for every row from one `fe_tag_select` call (matmul, per-tag max,
threshold, sort and top-k on the device; only ids and scores come back). facet_amd/tag_existing.py builds the reference's two library
loops on it.
"""
import numpy as np


def bytes_to_embedding(b):
    return np.frombuffer(b, dtype=np.float32)  # reference utils/embedding.py:26


class CLIPTagger:
    def __init__(self, clip_model=None, device='cuda', config=None):
        self.model, self.device, self.config = clip_model, device, config
        self.text_embeddings = None
        self.tag_names = None
        if config:
            self.tag_vocabulary = config.get_tag_vocabulary()
            self.art_tags = config.get_art_tags()
        else:
            self.tag_vocabulary, self.art_tags = {}, set()

    def prompts(self):
        """(tag_names, prompts) flattened like the reference (:60-66): one "a photo of {synonym}" per synonym."""
        names, texts = [], []
        for tag, descs in self.tag_vocabulary.items():
            for d in descs:
                names.append(tag)
                texts.append(f"a photo of {d}")
        return names, texts

    def precompute_text_embeddings(self, tokenizer):
        """Reference _precompute_text_embeddings (:51-75) with an injected tokenizer (open_clip.get_tokenizer('ViT-L-14')
        where available): prompts -> tokens -> clip_model.encode_text on the engine -> L2-normalised rows."""
        if self.model is None:
            return
        names, texts = self.prompts()
        feats = self.model.encode_text(tokenizer(texts))
        feats = feats.detach().cpu().numpy() if hasattr(feats, "detach") else np.asarray(feats)
        self.set_text_embeddings(names, feats)

    def set_text_embeddings(self, tag_names, embeddings):
        e = np.asarray(embeddings, np.float32)
        self.text_embeddings = e / np.linalg.norm(e, axis=-1, keepdims=True)
        self.tag_names = list(tag_names)

    def _tag_scores(self, clip_embedding_bytes):
        sims = self.text_embeddings @ bytes_to_embedding(clip_embedding_bytes).astype(np.float32)
        scores = {}
        for name, s in zip(self.tag_names, sims):
            if name not in scores or s > scores[name]:
                scores[name] = float(s)
        return scores

    def get_tags_from_embedding(self, clip_embedding_bytes, threshold=0.25, max_tags=5):
        if self.text_embeddings is None or clip_embedding_bytes is None:
            return []
        kept = [(t, s) for t, s in self._tag_scores(clip_embedding_bytes).items() if s >= threshold]
        kept.sort(key=lambda x: x[1], reverse=True)
        return [t for t, _ in kept[:max_tags]]

    def get_tags_batch(self, embeddings, engine, threshold=0.25, max_tags=5):
        """Batched form of get_tags_from_embedding: one GPU GEMM for all images ([n,768] array or list of blobs),
        then the reference's per-tag max / threshold / sort / top-k on the host."""
        if self.text_embeddings is None:
            return [[] for _ in embeddings]
        embs = np.stack([bytes_to_embedding(e) if isinstance(e, (bytes, bytearray)) else np.asarray(e, np.float32)
                         for e in embeddings]).astype(np.float32)
        sims = engine.tag_similarities(embs, self.text_embeddings)
        out = []
        for row in sims:
            scores = {}
            for name, s in zip(self.tag_names, row):
                if name not in scores or s > scores[name]:
                    scores[name] = float(s)
            kept = sorted(((t, s) for t, s in scores.items() if s >= threshold), key=lambda x: x[1], reverse=True)
            out.append([t for t, _ in kept[:max_tags]])
        return out

    # ---- the selection on the engine (fe_tag_select): similarities, per-tag max, threshold and top-k in one call ----------------------
    def use_engine(self, engine):
        """Sets the engine's tag vocabulary from tag_names / text_embeddings (packed once, Engine.tag_vocab) and keeps the engine for
        select_batch / scores_batch / is_artwork_batch. Tag ids are the tags in order of first appearance: the reference's dict order.
        Call it again after set_text_embeddings."""
        if self.text_embeddings is None:
            raise ValueError("use_engine: no text embeddings yet (set_text_embeddings / precompute_text_embeddings)")
        self._tag_list = list(dict.fromkeys(self.tag_names))
        index = {t: i for i, t in enumerate(self._tag_list)}
        engine.tag_vocab(self.text_embeddings, [index[t] for t in self.tag_names])
        self._engine = engine
        return self

    def _rows(self, embeddings):
        """[n,768] array, (device_ptr, n, ld), or a list of blobs / arrays (a blob of the wrong length raises ValueError with its index)."""
        if isinstance(embeddings, (tuple, np.ndarray)):
            return embeddings
        d = self.text_embeddings.shape[1]
        out = np.empty((len(embeddings), d), np.float32)
        for i, e in enumerate(embeddings):
            v = bytes_to_embedding(e) if isinstance(e, (bytes, bytearray, memoryview)) else np.asarray(e, np.float32).reshape(-1)
            if v.shape[0] != d:
                raise ValueError(f"embedding {i} has {v.shape[0]} floats, the vocabulary has {d}")
            out[i] = v
        return out

    def _select(self, embeddings, threshold, max_tags):
        engine = getattr(self, "_engine", None)
        if engine is None:
            raise RuntimeError("no engine: call use_engine(engine) first")
        rows = self._rows(embeddings)
        n = rows[1] if isinstance(rows, tuple) else len(rows)
        if n == 0:
            return np.empty((0, max_tags), np.int32), np.empty((0, max_tags), np.float32), np.empty(0, np.int32)
        return engine.tag_select(rows, threshold, min(int(max_tags), len(self._tag_list)))

    def select_batch(self, embeddings, threshold=0.25, max_tags=5):
        """get_tags_from_embedding for every row in one engine call -> list[list[str]]."""
        if self.text_embeddings is None:
            return [[] for _ in range(embeddings[1] if isinstance(embeddings, tuple) else len(embeddings))]
        if max_tags <= 0:      # the reference's slice [:max_tags]
            full = self.select_batch(embeddings, threshold, len(self._tag_list))
            return [t[:max_tags] for t in full]
        ids, _, counts = self._select(embeddings, threshold, max_tags)
        names = self._tag_list
        return [[names[g] for g in row[:c]] for row, c in zip(ids.tolist(), counts.tolist())]

    def scores_batch(self, embeddings, threshold=0.20):
        """get_tags_with_scores for every row in one engine call -> list[dict], each in vocabulary order with round(score, 3)."""
        if self.text_embeddings is None:
            return [{} for _ in range(embeddings[1] if isinstance(embeddings, tuple) else len(embeddings))]
        ids, scores, counts = self._select(embeddings, threshold, len(self._tag_list))
        names, out = self._tag_list, []
        for row, sc, c in zip(ids.tolist(), scores.tolist(), counts.tolist()):      # tolist: float32 -> the same value as a Python float
            kept = sorted(zip(row[:c], sc[:c]))
            out.append({names[g]: round(s, 3) for g, s in kept})
        return out

    def is_artwork_batch(self, embeddings, threshold=0.24):
        """is_artwork for every row in one engine call -> list[bool]."""
        return [bool(set(t) & self.art_tags) for t in self.select_batch(embeddings, threshold=threshold, max_tags=10)]

    def get_tags_with_scores(self, clip_embedding_bytes, threshold=0.20):
        if self.text_embeddings is None or clip_embedding_bytes is None:
            return {}
        return {t: round(s, 3) for t, s in self._tag_scores(clip_embedding_bytes).items() if s >= threshold}

    def is_artwork(self, clip_embedding_bytes, threshold=0.24):
        return bool(set(self.get_tags_from_embedding(clip_embedding_bytes, threshold=threshold, max_tags=10)) & self.art_tags)
