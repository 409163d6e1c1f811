"""Per-slide steps between a slide's uint8 patches and its cluster tokens, shared by the CLIs that run them one file at a
time (``cli.compute_features``, ``cli.kmean_features``) and by the path that runs them without a patch store
(``patchgen.embed_slide``, ``cli.slide_features``): one statement of each step, so the two routes cannot drift apart."""
import random


def sample_keys(keys, max_patch_number):
    """compute_features_hdf5.py:108-110: the patch names a slide contributes, in the order their features are stored -- all
    of ``keys`` as listed, or ``random.sample`` of them (the ``random`` module's global state, seeded by the caller) when
    there are more than ``max_patch_number``."""
    keys = list(keys)
    if len(keys) > max_patch_number:
        keys = random.sample(keys, max_patch_number)
    return keys


def patch_features(model, patches, feat_type, resize, device):
    """uint8 patches [n, H, W, 3] (host or device tensor) -> f32 [n, D] on the device: for ``feat_type`` "uni" and patches
    that are not 224 pixels the ``transforms.Resize(224)`` of compute_features_hdf5.py:54 first (``resize`` "pil": bit for
    bit PIL's BILINEAR, else the antialiased float interpolation), then the extractor with its transform fused."""
    if feat_type == 'uni' and patches.shape[1] != 224:
        if resize == 'pil':
            from .imgproc import resize_u8_pil
            patches = resize_u8_pil(patches.to(device), 224, "bilinear")
        else:
            from .uni import resize_u8
            patches = resize_u8(patches.to(device), 224)
    return model.extract_patches_u8(patches, sub_batch=1000)          # clamped per mode / patch size by the extractor


def cluster(features, num_clusters, random_state=0):
    """kmean_features.py:96-106 for one slide: f32 [n, D] on the device -> the dict of ``kmeans.kmeans_fit`` (labels [1, n],
    cluster_features [1, k, D], ...)."""
    from .kmeans import kmeans_fit
    return kmeans_fit(features, num_clusters, random_state=random_state)
