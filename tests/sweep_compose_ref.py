"""Host restatement of the composer at the swept depth defined in include/tscm/tscm.h (tscm_sweep_compose): the hypothesis
index of every pixel and the gather of the sweep tables along the hypothesis axis.  Everything behind the gather -- sample,
alpha, gain, label, coverage, SEAM, FEATHER, the MULTIBAND pyramids -- is tests/pano_ref.py, imported and not copied: a packed
record is a function of its table element alone, so the record (k, z(i, j)) at pixel (i, j) is the panorama's record of the
gathered table.  Integer arithmetic throughout, so the device result is compared with array_equal."""
import numpy as np

from tests import pano_ref

SEAM, FEATHER, MULTIBAND = pano_ref.SEAM, pano_ref.FEATHER, pano_ref.MULTIBAND


def hypothesis(index16, D: int, fallback_index: int = 0) -> np.ndarray:
    """z = index16 < 0 ? fallback_index : min(D - 1, (index16 + 8) >> 4), uint8 [ph, pw]"""
    idx = np.asarray(index16).astype(np.int64)
    assert 0 <= fallback_index < D
    return np.where(idx < 0, fallback_index, np.minimum(D - 1, (idx + 8) >> 4)).astype(np.uint8)


def gather(maps, z) -> np.ndarray:
    """maps [n, D, ph, pw], z [ph, pw] -> [n, ph, pw]: element (k, z(i, j), i, j)"""
    maps = np.asarray(maps)
    return np.take_along_axis(maps, np.asarray(z).astype(np.int64)[None, None], axis=1)[:, 0]


def compose(images, weights, mapx, mapy, index16, mode=MULTIBAND, levels=4, wrap=True, gains=None, fallback_index=0) -> dict:
    """Everything tscm_sweep_compose / _stages give for one frame: pano_ref.compose on the gathered tables, and the
    hypothesis plane.  images: n arrays [h, w] or [h, w, 3]; mapx, mapy: [n, D, ph, pw] float32; index16: int16 [ph, pw]."""
    z = hypothesis(index16, mapx.shape[1], fallback_index)
    res = pano_ref.compose(images, weights, gather(mapx, z), gather(mapy, z), mode=mode, levels=levels, wrap=wrap, gains=gains)
    res["hypothesis"] = z
    return res


def equirect_truth(shade, pano_w: int, pano_h: int, supersample: int = 4) -> np.ndarray:
    """What a camera at the rig origin sees on the equirect grid of maps.panorama_descs: shade(longitude, latitude) averaged
    over supersample x supersample positions inside every pixel, rounded to uint8."""
    offs = (np.arange(supersample) + 0.5) / supersample - 0.5
    jj, ii = np.meshgrid(np.arange(pano_w, dtype=np.float64), np.arange(pano_h, dtype=np.float64))
    acc = np.zeros((pano_h, pano_w))
    for oy in offs:
        for ox in offs:
            acc += shade((jj + ox - pano_w / 2.0) / (pano_w / (2 * np.pi)), (ii + oy - pano_h / 2.0) / (pano_h / np.pi))
    return np.clip(np.rint(acc / supersample ** 2), 0, 255).astype(np.uint8)


def mean_abs_error(pano, truth) -> float:
    return float(np.mean(np.abs(np.asarray(pano).astype(np.int64).reshape(truth.shape) - truth.astype(np.int64))))
