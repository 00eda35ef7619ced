"""The batch step: what reference processing/batch_processor.py `_process_batch` (:169-360) and the multi-pass `_pass_*`
functions (processing/multi_pass.py:481-644) sequence per image - one model after another, one image after another - as a
handful of engine calls over a whole same-sized batch.

    BatchScorer(engine, tagger=None, face_analyzer=None).process_batch(images_rgb) -> list[dict]

Each dict carries, under the reference's own key names (batch_processor.py:298-354), every value that comes out of a model or
a pixel scan: CLIP aesthetic + embedding blob, TOPIQ quality, SAMP-Net composition score / pattern, the face dict's fields,
the seven technical-metric groups, tags, and the two cross terms the reference derives on the spot (face_ratio :244,
isolation_bonus :264-269). What stays with the caller because it needs files, configuration policy or libraries outside the
hot path: path / EXIF columns, leading lines (CompositionAnalyzer.detect_leading_lines: Canny + probabilistic
Hough; `detect_lines=True` computes them through `fe_leading_lines`, or pass `leading_lines=` scores in). `phash=True` adds the
`phash` column (`str(imagehash.phash(pil_img))`, batch_processor.py:216) through `fe_phash`; off by default. `thumbnails=True` adds the
`thumbnail` column (`generate_photo_thumbnail(pil_img, 640, 80)`, scorer.py:1611-1617: JPEG bytes) through `fe_thumbnail_jpeg`; off by default.
`subject_region=True` makes power_point_score and the rule-based comp_score those of the multi-pass path (multi_pass.py:685-701:
placement of the subject box `CompositionAnalyzer.detect_subject_region` finds in the image) through `fe_subject_region`; off by default. With `policy=` (an `aggregate.AggregatePolicy` made from the
scoring configuration) the category and aggregate score (`Facet.calculate_aggregate_logic`) are computed for the whole batch
as the last step, from the multi-pass metrics mapping (multi_pass.py:713-752); `metrics_for_aggregate()` returns the
narrower mapping of the single-pass path (batch_processor.py:272-296).

Engine calls per batch: fe_ensemble_score (TOPIQ + CLIP + aesthetic + U2-Net-P + SAMP-Net), fe_image_stats (technical scans),
fe_face_analyze + fe_roi_laplacian (+ fe_face_thumbnails with `gpu_thumbnails=True`; through FaceAnalyzer.analyze_faces_batch), fe_tag_similarities (through CLIPTagger; with `gpu_tag_select=True`
fe_tag_select instead: the tags' selection on the device too, CLIPTagger.select_batch),
fe_phash (with `phash=True`), fe_thumbnail_jpeg (with `thumbnails=True`), fe_subject_region (with `subject_region=True`).

Mixed sizes: `process_images` / `process_files` take a chunk of photos of any sizes. By default the chunk is cut into one process_batch
per distinct shape. `mixed_sizes=True` uploads the chunk once and scores all of it with ONE fe_ensemble_score_mixed call (CLIP and SAMP
crops gather across shapes into the towers' usual chunks; TOPIQ runs per shape group inside that call) and computes the technical
statistics of all of it with ONE fe_image_stats_mixed call on the RGB pixels. With `thumbnails=True` the thumbnails of the whole chunk come
from ONE fe_thumbnail_jpeg_mixed call and, with `phash=True` as well, its hashes from ONE fe_phash_mixed call, both on the RGB pixels and
both without a per-size table left in the context. With a face analyzer the face dicts of the whole chunk come from ONE
fe_face_analyze_mixed call, ONE fe_roi_laplacian_mixed call and (with `gpu_thumbnails=True`) ONE fe_face_thumbnails_mixed call, again on the
RGB pixels: every face graph runs over full micro-batches whatever the shapes. With `detect_lines=True` the line scores of the whole chunk
come from ONE fe_leading_lines_mixed call and with `subject_region=True` its subject boxes from ONE fe_subject_region_mixed call, both on
the RGB pixels. No stage of a mixed chunk asks for a BGR copy of the resident pixels any more, except pHash without thumbnails, which
keeps its per-group fe_phash on one; the dicts come back in input order with the same keys and values.

Overlap: a context runs one call at a time (one arena, one stream), and the face / statistics / leading-lines calls spend most of
their time in host glue (NMS, similarity transforms, Hough votes, percentile arithmetic) with the GPU idle. Give the scorer a second
context on the same GPU (`aux_engine=`, and build the FaceAnalyzer on it): those calls then run on a worker thread beside
fe_ensemble_score - ctypes drops the GIL, the hardware queues interleave the two streams - and the step costs max(models, rest)
instead of their sum. Results are identical to the single-context path (tests/test_batch_gpu.py).
"""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .aggregate import aggregate_batch
from .image_stats import TechnicalAnalyzer
from .samp_net import postprocess as samp_postprocess


def tags_to_string(tags):
    """utils/tags.py:8-20."""
    return ','.join(tags) if tags else None


def placement_data(bbox, img_w, img_h, power_weight=2.0, line_weight=1.0):
    """CompositionAnalyzer.get_placement_data(bbox, w, h, config) as `_process_batch` calls it (batch_processor.py:245-247, without
    img_cv): rule-of-thirds power points / lines vs centred composition; analyzers/composition.py:111-187. The two weights are
    config.get_composition_weights()'s power_point_weight / line_weight."""
    if bbox is None:
        return {'score': 7.0, 'power_point_score': 5.0, 'line_score': 5.0, 'center_score': 7.0}
    cx = (bbox[0] + bbox[2]) / 2 / img_w
    cy = (bbox[1] + bbox[3]) / 2 / img_h
    thirds = [1 / 3, 2 / 3]
    nearest_pp = min(np.sqrt((cx - px) ** 2 + (cy - py) ** 2) for px in thirds for py in thirds)
    pp = max(0, 10 - nearest_pp * 25)
    line = max(0, 10 - (min(abs(cx - t) for t in thirds) + min(abs(cy - t) for t in thirds)) * 15)
    centre = max(0, 10 - (abs(cx - 0.5) + abs(cy - 0.5)) * 10)
    best = max((pp * power_weight + line * line_weight) / (power_weight + line_weight), centre)
    return {'score': round(best, 2), 'power_point_score': round(pp, 2), 'line_score': round(line, 2), 'center_score': round(centre, 2)}


def detect_silhouette(histogram_silhouette, tags, face_count):
    """utils/detection.py:8-29: (histogram silhouette or a 'silhouette' tag) and a human (a face, or a portrait / group tag).
    `tags` is the comma-joined tag string (substring tests, as in the reference)."""
    tagged = ('silhouette' in tags) if tags else False
    human = face_count > 0 or (any(t in tags for t in ('portrait', 'group')) if tags else False)
    return 1 if ((histogram_silhouette or tagged) and human) else 0


class BatchScorer:
    def __init__(self, engine, tagger=None, face_analyzer=None, tag_threshold=0.22, max_tags=5, mono_threshold=0.10,
                 shadow_threshold=0.15, highlight_threshold=0.10, power_weight=2.0, line_weight=1.0, policy=None, detect_lines=False,
                 aux_engine=None, phash=False, vlm_composition=None, thumbnails=False, thumbnail_size=640, thumbnail_quality=80,
                 subject_region=False, mixed_sizes=False, gpu_tag_select=False):
        # tags from CLIPTagger.select_batch (fe_tag_select: per-tag max, threshold and top-k on the device; the similarities stay there)
        # instead of get_tags_batch (GEMM on the device, the [n, T] matrix back, the selection in Python). Off by default.
        self.gpu_tag_select = gpu_tag_select
        # process_images / process_files: one fe_ensemble_score_mixed call for the whole chunk instead of one fe_ensemble_score per distinct
        # shape (module docstring, "Mixed sizes"). Off by default.
        self.mixed_sizes = mixed_sizes
        # multi-pass placement (multi_pass.py:685-701): get_placement_data(None, w, h, config, img_cv) - the subject box detected from the
        # resident BGR copy (fe_subject_region) is what power_point_score and the rule-based comp_score are computed from, faces or not
        self.subject_region = subject_region
        # Qwen2-VL composition analyzer (facet_amd/vlm_composition.py; the 24gb profile): its SCORE overwrites comp_score, scorer.py:698-705
        self.vlm_composition = vlm_composition
        self.phash = phash      # add the 'phash' column (16 hex digits) from the resident BGR copy
        # add the 'thumbnail' column (JPEG bytes, generate_photo_thumbnail(pil_img, size, quality)) from the resident BGR copy
        self.thumbnails, self.thumbnail_size, self.thumbnail_quality = thumbnails, thumbnail_size, thumbnail_quality
        self.engine, self.tagger, self.face_analyzer, self.policy, self.detect_lines = engine, tagger, face_analyzer, policy, detect_lines
        # second context on the same GPU for statistics / faces / lines (see module docstring); None = everything on `engine`, in sequence
        self.aux_engine = aux_engine
        self._pool = ThreadPoolExecutor(max_workers=1) if aux_engine is not None else None
        if aux_engine is not None and face_analyzer is not None and getattr(face_analyzer, "available", False):
            fe = getattr(getattr(face_analyzer, "face_app", None), "engine", None)
            if fe is not None and fe is engine:
                raise ValueError("with aux_engine the FaceAnalyzer must be built on the aux engine (one call at a time per context)")
        self.power_weight, self.line_weight = power_weight, line_weight
        self.tag_threshold, self.max_tags = tag_threshold, max_tags           # utils/tags.py:50-51 defaults
        self.mono_threshold, self.shadow_threshold, self.highlight_threshold = mono_threshold, shadow_threshold, highlight_threshold

    def process_batch(self, images_rgb, exif=None, leading_lines=None, _resident=None, _records=None, _borrowed=False, _tech=None, _hashes=None,
                      _thumbs=None, _faces=None, _subjects=None):
        """images_rgb: uint8 [n,h,w,3] (the PIL images of a batch as one array). Returns one dict per image. exif: optional list
        of per-image dicts (iso / f_stop / shutter_speed / focal_length) and leading_lines: optional per-image
        leading_lines_score, both only used by the aggregate step (policy given).
        _resident (process_files): (device_ptr, n, h, w) of an RGB batch that is already on the device, handed over - it is freed here -
        with images_rgb None; the pixels are fetched only when a stage that works on host arrays (face thumbnails cut by Pillow, the VLM analyzer) is on.
        _records (the mixed-size path): (records [n, 789], mask) of these images, computed by the caller - the ensemble call is skipped.
        _borrowed: the resident batch stays the caller's and is not freed here.
        _tech (the mixed-size path): the technical dicts of these images (TechnicalAnalyzer.analyze_mixed), computed by the caller - the
        statistics call is skipped, and the BGR copy is made only when a stage that reads it is on.
        _hashes / _thumbs (the mixed-size path): the phash strings / thumbnail bytes of these images (fe_phash_mixed, fe_thumbnail_jpeg_mixed),
        computed by the caller - that stage is skipped and asks for no BGR copy.
        _faces (the mixed-size path): the face dicts of these images (FaceAnalyzer.analyze_faces_mixed), computed by the caller - the face
        calls are skipped, ask for no BGR copy and for no host pixels.
        _subjects (the mixed-size path): the subject boxes of these images (CompositionAnalyzer.detect_subject_region_mixed), computed by
        the caller - fe_subject_region is skipped and asks for no BGR copy. (The line scores of that path come in through leading_lines.)"""
        e = self.engine
        if _resident is None:
            imgs = np.ascontiguousarray(images_rgb, dtype=np.uint8)
            n, h, w, _ = imgs.shape
            d_rgb = e.dev_alloc(imgs.nbytes)
        else:
            imgs = None
            d_rgb, n, h, w = _resident
        d_bgr = None
        try:
            # one upload; the BGR copy the reference keeps as img_cv is made on the device, and every engine call reads the resident batch
            if _resident is None:
                e.h2d(d_rgb, imgs)
            elif (_faces is None and self.face_analyzer is not None and self.face_analyzer.available and
                  not getattr(self.face_analyzer, 'gpu_thumbnails', False)) or self.vlm_composition is not None:      # face thumbnails cut on the engine need no host pixels
                imgs = np.empty((n, h, w, 3), np.uint8)
                e.d2h(imgs, d_rgb)
            faces_on = self.face_analyzer is not None and self.face_analyzer.available
            bgr_dev = None
            if _tech is None or (faces_on and _faces is None) or (leading_lines is None and self.detect_lines) or (self.phash and _hashes is None) or \
                    (self.thumbnails and _thumbs is None) or (self.subject_region and _subjects is None):
                d_bgr = e.dev_alloc(n * h * w * 3)
                e.swap_rb(d_rgb, n * h * w, d_bgr)
                bgr_dev = (d_bgr, n, h, w)
            rgb_dev = (d_rgb, n, h, w)

            def rest(eng):      # everything that is not a model of the ensemble; reads the BGR copy only
                tech_ = _tech
                if tech_ is None:
                    tech_ = TechnicalAnalyzer.analyze_batch(eng, bgr_dev, self.shadow_threshold, self.highlight_threshold, self.mono_threshold)
                faces_ = _faces
                if faces_on and faces_ is None:
                    faces_ = self.face_analyzer.analyze_faces_batch([imgs[i][..., ::-1] for i in range(n)] if imgs is not None else None,
                                                                    resident=bgr_dev)
                lines_ = leading_lines
                if lines_ is None and self.detect_lines:      # CompositionAnalyzer.detect_leading_lines (multi_pass.py:702-705), batched
                    from .composition import score_lines
                    lines_ = [score_lines(l, h, w)['leading_lines_score'] for l in eng.leading_lines(bgr_dev)]
                hashes_ = _hashes
                if self.phash and hashes_ is None:      # the same bytes as the PIL image, in B,G,R order
                    from .phash import phash_batch
                    hashes_ = phash_batch(eng, bgr_dev, bgr=True)
                thumbs_ = _thumbs
                if self.thumbnails and thumbs_ is None:
                    from .thumbnail import thumbnails
                    thumbs_ = thumbnails(eng, bgr_dev, self.thumbnail_size, self.thumbnail_quality, bgr=True)
                subjects_ = _subjects
                if self.subject_region and subjects_ is None:
                    from .composition import CompositionAnalyzer
                    subjects_ = CompositionAnalyzer.detect_subject_region_batch(eng, bgr_dev)
                return tech_, faces_, lines_, hashes_, thumbs_, subjects_

            if _records is not None:
                rec, mask = _records
                tech, faces, leading_lines, hashes, thumbs, subjects = rest(self.aux_engine if self._pool is not None else e)
            elif self._pool is not None:
                fut = self._pool.submit(rest, self.aux_engine)      # fe_swap_rb_u8 has synchronised: the BGR copy is complete
                try:
                    rec, mask = e.ensemble_score(rgb_dev)
                finally:
                    tech, faces, leading_lines, hashes, thumbs, subjects = fut.result()      # also on error: the worker must be done before the buffers go
            else:
                rec, mask = e.ensemble_score(rgb_dev)
                tech, faces, leading_lines, hashes, thumbs, subjects = rest(e)
        finally:
            if not _borrowed:
                e.dev_free(d_rgb)
            if d_bgr is not None:
                e.dev_free(d_bgr)
        tags = None
        if self.tagger is not None and self.tagger.text_embeddings is not None and mask & 2:
            if self.gpu_tag_select:
                if getattr(self.tagger, '_engine', None) is not self.engine:
                    self.tagger.use_engine(self.engine)
                tags = self.tagger.select_batch(rec[:, 21:789], self.tag_threshold, self.max_tags)
            else:
                tags = self.tagger.get_tags_batch(rec[:, 21:789], self.engine, self.tag_threshold, self.max_tags)
        out = []
        for i in range(n):
            t = tech[i]
            res = {'image_width': w, 'image_height': h}
            if mask & 2:          # CLIP + aesthetic head: Facet.get_aesthetic_and_quality_batch (scorer.py:640-673)
                aesthetic = max(0.0, min(10.0, (float(rec[i, 1]) + 1) * 5))
                res.update({'aesthetic': round(aesthetic, 2), 'clip_embedding': rec[i, 21:789].astype(np.float32).tobytes(),
                            'scoring_model': 'clip-mlp'})
            res['quality_score'] = None
            if mask & 1:          # TOPIQ pass (multi_pass.py:631-642): normalised score (pyiqa_scorer.py:166-195: clamp to [0,1], x10)
                q = max(0.0, min(10.0, max(0.0, min(1.0, float(rec[i, 0]))) * 10.0))      # becomes aesthetic AND quality_score
                if 'aesthetic' in res:
                    res['clip_aesthetic'] = res['aesthetic']
                res.update({'aesthetic': round(q, 2), 'quality_score': q, 'scoring_model': 'topiq'})
            if mask & 4:          # SAMP-Net: get_composition_scores (scorer.py:675-700) overwrites comp_data['score']
                sp = samp_postprocess(rec[i, 2:10], rec[i, 10:16], rec[i, 16:21])
                res.update({'comp_score': round(sp['comp_score'], 2), 'composition_pattern': sp['pattern']})
            res.update({
                'tech_sharpness': round(t['sharpness']['normalized'], 2), 'raw_sharpness_variance': float(t['sharpness']['raw_variance']),
                'color_score': round(t['color']['normalized'], 2), 'raw_color_entropy': float(t['color']['raw_entropy']),
                'exposure_score': round(t['histogram']['exposure_score'], 2), 'histogram_data': t['histogram']['histogram_bytes'],
                'histogram_spread': float(t['histogram']['spread']), 'mean_luminance': float(t['histogram']['mean_luminance']),
                'histogram_bimodality': float(t['histogram']['bimodality']), 'shadow_clipped': t['histogram'].get('shadow_clipped', 0),
                'highlight_clipped': t['histogram'].get('highlight_clipped', 0), 'is_monochrome': t['mono']['is_monochrome'],
                'mean_saturation': t['mono']['mean_saturation'], 'dynamic_range_stops': t['dynamic_range']['dynamic_range_stops'],
                'noise_sigma': t['noise']['noise_sigma'], 'contrast_score': t['contrast']['contrast_score'],
            })
            res['tags'] = tags_to_string(tags[i]) if tags is not None else None
            if faces is not None:
                f = faces[i]
                isolation, blink = 1.0, 0
                if f['face_count'] > 0:      # batch_processor.py:264-269
                    isolation = max(1.0, f['face_sharpness'] / (t['cache'].laplacian_variance + 1))
                    blink = f.get('is_blink', 0)
                res.update({'face_count': f['face_count'], 'face_quality': f['face_quality'], 'eye_sharpness': f['eye_sharpness'],
                            'face_sharpness': f['face_sharpness'], 'face_ratio': f.get('face_area', 0) / (h * w),
                            'raw_eye_sharpness': float(f.get('raw_eye_sharpness', 0)), 'is_group_portrait': f.get('is_group_portrait', 0),
                            'face_confidence': f.get('max_face_confidence', 0), 'isolation_bonus': round(isolation, 2), 'is_blink': blink,
                            'face_details': f.get('face_details', []), '_face_bbox': f.get('bbox'), '_isolation_bonus_raw': isolation})
            # rule-based placement of the (union) face box, then SAMP-Net's score on top when it ran (scorer.py:675-690)
            comp = placement_data(subjects[i] if subjects is not None else res.get('_face_bbox'), w, h, self.power_weight, self.line_weight)
            res['power_point_score'] = float(comp['power_point_score'])
            res.setdefault('comp_score', round(comp['score'], 2))
            res['is_silhouette'] = detect_silhouette(t['histogram'].get('is_silhouette', 0), res.get('tags'), res.get('face_count', 0))
            if leading_lines is not None:
                res['leading_lines_score'] = float(leading_lines[i])
            if hashes is not None:
                res['phash'] = hashes[i]
            if thumbs is not None:
                res['thumbnail'] = thumbs[i]
            out.append(res)
        if self.vlm_composition is not None:
            self.apply_vlm_composition(out, imgs)
        if self.policy is not None:
            rows = [self.metrics_multi_pass(r, exif[i] if exif else None) for i, r in enumerate(out)]
            scores, cats = aggregate_batch(rows, self.policy)
            for r, s, c in zip(out, scores.tolist(), cats):
                r['aggregate'], r['category'] = s, c
        return out

    def apply_vlm_composition(self, results, images_rgb):
        """The VLM step of Facet.get_composition_scores (scorer.py:698-705), after the SAMP step: one batch_analyze for the batch; each dict
        takes comp_score from the analyzer's score (rounded to 2 decimals like every comp_score the batch step stores,
        batch_processor.py:313) and gains composition_explanation (batch_processor.py:348). A result without a score leaves its dict alone."""
        from PIL import Image
        for res, r in zip(results, self.vlm_composition.batch_analyze([Image.fromarray(np.asarray(a, np.uint8)) for a in images_rgb])):
            if r.get('composition_score') is not None:
                res['comp_score'] = round(float(r['composition_score']), 2)
                res['composition_explanation'] = r.get('explanation')
        return results

    def process_images(self, images_rgb, exif=None, leading_lines=None):
        """Images of ANY sizes (a list of uint8 [h,w,3] arrays / PIL images, as a chunk of the reference's loader holds them): grouped by
        shape, each group goes through process_batch as one resident batch; results come back in input order."""
        arrs = [np.asarray(im.convert('RGB') if hasattr(im, 'convert') else im, dtype=np.uint8) for im in images_rgb]
        groups = {}
        for i, a in enumerate(arrs):
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"image {i}: expected [h,w,3], got {a.shape}")
            groups.setdefault(a.shape, []).append(i)
        out = [None] * len(arrs)
        if self.mixed_sizes and arrs:
            return self._process_images_mixed(arrs, groups, exif, leading_lines)
        for idx in groups.values():
            res = self.process_batch(np.stack([arrs[i] for i in idx]), exif=[exif[i] for i in idx] if exif else None,
                                     leading_lines=[leading_lines[i] for i in idx] if leading_lines is not None else None)
            for i, r in zip(idx, res):
                out[i] = r
        return out

    def _process_images_mixed(self, arrs, groups, exif, leading_lines, out=None, index=None):
        """The chunk goes up once, into one allocation in which every shape group lies back to back (256-byte aligned), and through
        _process_mixed. index: the callers' indices of arrs (process_files), default 0 .. len(arrs) - 1."""
        e = self.engine
        index = list(range(len(arrs))) if index is None else index
        out = [None] * len(arrs) if out is None else out
        at, starts = 0, []
        for (h, w, _), idx in groups.items():
            starts.append(at)
            at += -(-(len(idx) * h * w * 3) // 256) * 256
        d_all = e.dev_alloc(at)
        try:
            entries = []
            for ((h, w, _), idx), a0 in zip(groups.items(), starts):
                dev = ctypes.c_void_p(d_all.value + a0)
                e.h2d(dev, np.stack([arrs[i] for i in idx]))
                entries.append(([index[i] for i in idx], (dev, len(idx), h, w), False))
            self._process_mixed(entries, out, exif, leading_lines)
        finally:
            e.dev_free(d_all)
        return out

    def _process_mixed(self, entries, out, exif, leading_lines):
        """entries: [(indices into out, (device_ptr, k, h, w), owned)] - resident RGB batches of one shape each. One ensemble_score_mixed call,
        one analyze_mixed call and, with a face analyzer, one analyze_faces_mixed call over every image of every entry, by pointers into the
        resident batches (all but the first on the aux engine's worker beside the first when there is one); then process_batch per entry
        for the stages that run per shape, with its records, technical dicts and face dicts handed in. An owned batch is freed by
        process_batch (or here, when the ensemble call fails)."""
        e = self.engine
        order, ptrs, sizes = [], [], []
        for idx, (p, k, h, w), _ in entries:
            base = p.value if isinstance(p, ctypes.c_void_p) else int(p)
            for j, i in enumerate(idx):
                order.append(i); ptrs.append(base + j * h * w * 3); sizes.append((h, w))
        by_input = sorted(range(len(order)), key=lambda r: order[r])      # the calls see the images in input order
        resident = ([ptrs[r] for r in by_input], [sizes[r] for r in by_input])

        fa = self.face_analyzer if (self.face_analyzer is not None and self.face_analyzer.available) else None
        host_bgr = None      # the chunk's host pixels as B,G,R views in input order, fetched below only when Pillow cuts the face thumbnails

        def stats(eng):      # one fe_image_stats_mixed over the whole chunk, straight from the RGB pixels; then the faces, the index columns, lines and subject boxes
            tech_ = TechnicalAnalyzer.analyze_mixed(eng, resident, self.shadow_threshold, self.highlight_threshold, self.mono_threshold, order='rgb')
            # the face dicts of the whole chunk (the analyzer holds its own context: the aux engine when there is one), R,G,B read in place
            faces_ = fa.analyze_faces_mixed(host_bgr, resident=resident, order='rgb') if fa is not None else None
            hashes_ = thumbs_ = None
            # Indexing (thumbnails on, the reference's two columns per photo): one fe_thumbnail_jpeg_mixed and, with phash on, one
            # fe_phash_mixed over the whole chunk, R,G,B read in place, so neither asks process_batch for a BGR copy. pHash without
            # thumbnails keeps its per-group fe_phash on the BGR copy: tests/test_stats_mixed_gpu.py pins that configuration's calls.
            if self.thumbnails:
                from .thumbnail import thumbnails_mixed
                thumbs_ = thumbnails_mixed(eng, resident, self.thumbnail_size, self.thumbnail_quality, order='rgb')
                if self.phash:
                    from .phash import phash_mixed, to_hex
                    hashes_ = to_hex(phash_mixed(eng, resident, order='rgb'))
            # Composition: one fe_leading_lines_mixed (unless the caller passed scores in) and one fe_subject_region_mixed over the whole
            # chunk, R,G,B read in place, so neither asks process_batch for a BGR copy
            lines_, subjects_ = leading_lines, None
            if self.detect_lines and lines_ is None:
                from .composition import CompositionAnalyzer
                lines_ = [d['leading_lines_score'] for d in CompositionAnalyzer.detect_leading_lines_mixed(eng, resident, order='rgb')]
                lines_ = dict(zip(sorted(order), lines_))      # by the caller's index, as leading_lines= is
            if self.subject_region:
                from .composition import CompositionAnalyzer
                subjects_ = CompositionAnalyzer.detect_subject_region_mixed(eng, resident, order='rgb')
            return tech_, hashes_, thumbs_, faces_, lines_, subjects_

        try:
            if fa is not None and not getattr(fa, 'gpu_thumbnails', False):
                views = {}
                for idx, (p, k, h, w), _ in entries:
                    a = np.empty((k, h, w, 3), np.uint8)
                    e.d2h(a, p)
                    views.update((i, a[j][..., ::-1]) for j, i in enumerate(idx))
                host_bgr = [views[order[r]] for r in by_input]
            if self._pool is not None:      # beside the ensemble call, on the aux context (module docstring, "Overlap")
                e.sync()                    # whatever filled the resident batches on this context's stream is complete
                fut = self._pool.submit(stats, self.aux_engine)
                try:
                    rec, mask = e.ensemble_score_mixed(resident)
                finally:
                    tech, hashes, thumbs, faces, leading_lines, subjects = fut.result()      # also on error: the worker must be done before the buffers go
            else:
                rec, mask = e.ensemble_score_mixed(resident)
                tech, hashes, thumbs, faces, leading_lines, subjects = stats(e)
        except Exception:
            for _, dev, owned in entries:
                if owned:
                    e.dev_free(dev[0])
            raise
        row = {order[r]: q for q, r in enumerate(by_input)}
        for n_done, (idx, dev, owned) in enumerate(entries):
            try:
                res = self.process_batch(None, exif=[exif[i] for i in idx] if exif else None,
                                         leading_lines=[leading_lines[i] for i in idx] if leading_lines is not None else None, _resident=dev,
                                         _records=(rec[[row[i] for i in idx]], mask), _borrowed=not owned, _tech=[tech[row[i]] for i in idx],
                                         _hashes=[hashes[row[i]] for i in idx] if hashes is not None else None,
                                         _thumbs=[thumbs[row[i]] for i in idx] if thumbs is not None else None,
                                         _faces=[faces[row[i]] for i in idx] if faces is not None else None,
                                         _subjects=[subjects[row[i]] for i in idx] if subjects is not None else None)
            except Exception:
                for _, dev2, owned2 in entries[n_done + 1:]:
                    if owned2:
                        e.dev_free(dev2[0])
                raise
            for i, r in zip(idx, res):
                out[i] = r

    def process_files(self, paths_or_blobs, exif=None, leading_lines=None, progressive=False, parallel_entropy=False):
        """Image FILES (paths, or the files' bytes) instead of decoded arrays: the reference's `_load_images` + batch step. JPEG files the
        engine decodes (facet_amd.image_loading) are decoded on the device per output size and scored from that resident batch, with no
        copy of the pixels down and up again; every other file is opened with Pillow as load_image_from_path does and goes through
        process_images. Results come back in input order; a file the reference could not load gives None. progressive=True: complete
        progressive files join the resident batch of their size instead of going through Pillow; the records are the same either way.
        parallel_entropy=True: the decoder works inside a file's entropy-coded segments in parallel (Engine.jpeg_decode); the same records again."""
        from .image_loading import decode_groups, pillow_rgb, read_blob
        blobs = [read_blob(p) for p in paths_or_blobs]
        out = [None] * len(blobs)
        e = self.engine
        groups, rest = decode_groups(e, blobs, device=True, progressive=progressive, parallel_entropy=parallel_entropy)
        if self.mixed_sizes:
            return self._process_files_mixed(blobs, groups, rest, out, exif, leading_lines)
        for idx, dev in groups:
            res = self.process_batch(None, exif=[exif[i] for i in idx] if exif else None,
                                     leading_lines=[leading_lines[i] for i in idx] if leading_lines is not None else None, _resident=dev)
            for i, r in zip(idx, res):
                out[i] = r
        arrs = [(i, pillow_rgb(blobs[i])) for i in rest]
        arrs = [(i, a) for i, a in arrs if a is not None]
        if arrs:
            idx = [i for i, _ in arrs]
            res = self.process_images([a for _, a in arrs], exif=[exif[i] for i in idx] if exif else None,
                                      leading_lines=[leading_lines[i] for i in idx] if leading_lines is not None else None)
            for i, r in zip(idx, res):
                out[i] = r
        return out

    def _process_files_mixed(self, blobs, groups, rest, out, exif, leading_lines):
        """process_files with mixed_sizes: the decode groups' resident buffers and one upload of the files Pillow opened go through a single
        ensemble_score_mixed call."""
        from .image_loading import pillow_rgb
        e = self.engine
        entries = [(idx, dev, True) for idx, dev in groups]
        arrs = [(i, pillow_rgb(blobs[i])) for i in rest]
        arrs = [(i, np.ascontiguousarray(a, dtype=np.uint8)) for i, a in arrs if a is not None]
        d_all = None
        try:
            if arrs:
                shapes = {}
                for r, (_, a) in enumerate(arrs):
                    shapes.setdefault(a.shape, []).append(r)
                at, starts = 0, []
                for (h, w, _), rs in shapes.items():
                    starts.append(at)
                    at += -(-(len(rs) * h * w * 3) // 256) * 256
                try:
                    d_all = e.dev_alloc(at)
                    for ((h, w, _), rs), a0 in zip(shapes.items(), starts):
                        dev = ctypes.c_void_p(d_all.value + a0)
                        e.h2d(dev, np.stack([arrs[r][1] for r in rs]))
                        entries.append(([arrs[r][0] for r in rs], (dev, len(rs), h, w), False))
                except Exception:
                    for _, dev, owned in entries:
                        if owned:
                            e.dev_free(dev[0])
                    raise
            if entries:
                self._process_mixed(entries, out, exif, leading_lines)
        finally:
            if d_all is not None:
                e.dev_free(d_all)
        return out

    @staticmethod
    def metrics_multi_pass(res, exif=None):
        """The `metrics` mapping of the multi-pass path (multi_pass.py:713-752) from a process_batch dict."""
        exif = exif or {}
        return {
            'aesthetic': res.get('aesthetic', 5.0), 'quality_score': res.get('quality_score'), 'scoring_model': res.get('scoring_model', 'clip-mlp'),
            'comp_score': res.get('comp_score', 5.0), 'face_count': res.get('face_count', 0), 'face_quality': res.get('face_quality', 0),
            'eye_sharpness': res.get('eye_sharpness', 0), 'face_sharpness': res.get('face_sharpness', 0), 'tech_sharpness': res['tech_sharpness'],
            'color_score': res['color_score'], 'exposure_score': res['exposure_score'], 'face_ratio': res.get('face_ratio', 0),
            'tags': res.get('tags') or '', 'isolation_bonus': res.get('_isolation_bonus_raw', 1.0), 'is_blink': res.get('is_blink', 0),
            'is_group_portrait': res.get('is_group_portrait', 0), 'shadow_clipped': res['shadow_clipped'], 'highlight_clipped': res['highlight_clipped'],
            'is_silhouette': res.get('is_silhouette', 0), 'histogram_spread': res['histogram_spread'], 'histogram_bimodality': res['histogram_bimodality'],
            'mean_luminance': res['mean_luminance'], 'is_monochrome': res['is_monochrome'], 'mean_saturation': res['mean_saturation'],
            'contrast_score': res['contrast_score'], 'noise_sigma': res['noise_sigma'], 'leading_lines_score': res.get('leading_lines_score', 0),
            'power_point_score': res.get('power_point_score', 5.0), 'topiq_score': res.get('quality_score'),
            'iso': exif.get('iso'), 'f_stop': exif.get('f_stop'), 'shutter_speed': exif.get('shutter_speed'), 'focal_length': exif.get('focal_length'),
        }

    @staticmethod
    def metrics_for_aggregate(res, exif=None, is_silhouette=None, comp_score=None):
        """The `metrics` mapping `Facet.calculate_aggregate_logic` is called with (batch_processor.py:272-296), built from a
        process_batch dict. comp_score: the caller's rule-based placement score when SAMP-Net is not loaded."""
        exif = exif or {}
        return {
            'aesthetic': res.get('aesthetic'), 'face_count': res.get('face_count', 0), 'face_quality': res.get('face_quality', 0),
            'eye_sharpness': res.get('eye_sharpness', 0), 'tech_sharpness': res['tech_sharpness'], 'color_score': res['color_score'],
            'exposure_score': res['exposure_score'], 'face_ratio': res.get('face_ratio', 0),
            'comp_score': res.get('comp_score', comp_score), 'isolation_bonus': res.get('_isolation_bonus_raw', 1.0),
            'is_blink': res.get('is_blink', 0), 'shadow_clipped': res['shadow_clipped'], 'highlight_clipped': res['highlight_clipped'],
            'is_silhouette': res.get('is_silhouette', 0) if is_silhouette is None else is_silhouette, 'histogram_spread': res['histogram_spread'], 'iso': exif.get('iso'), 'f_stop': exif.get('f_stop'),
            'quality_score': res.get('quality_score'), 'scoring_model': res.get('scoring_model', 'clip-mlp'),
        }
