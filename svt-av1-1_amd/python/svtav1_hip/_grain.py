"""AV1 film-grain synthesis (svthip_film_grain_tables_dev, svthip_av1_[highbd_]add_film_grain_dev) and estimation
(svthip_[highbd_]film_grain_noise_model_dev, svthip_film_grain_flat_block_tables_dev, svthip_[highbd_]film_grain_flat_block_features_dev) and Wiener denoising (svthip_[highbd_]film_grain_wiener_filter_dev, _dither_dev,
_wiener_denoise_dev): pointer marshalling only.

The parameter block svthip_film_grain_params crosses Python as a packed buffer built by film_grain_params(**fields): the layout of
aom_film_grain_t, all int32 in declaration order, then the uint16 random_seed and a reserved uint16."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from . import _abi
from ._core import _check, lib

_LAYOUT = _abi.dtype("svthip_film_grain_params")
# (field, struct code, number of values) in the order of the C struct; a [n][2] array of scaling points counts 2 n
_FILM_GRAIN_FIELDS = [(name, _LAYOUT[name].base.char, int(np.prod(_LAYOUT[name].shape, dtype=int))) for name in _LAYOUT.names]
_PACKED = "<" + "".join(f"{n}{code}" for _, code, n in _FILM_GRAIN_FIELDS)
FILM_GRAIN_PARAMS_BYTES = _LAYOUT.itemsize
assert struct.calcsize(_PACKED) == FILM_GRAIN_PARAMS_BYTES   # the C struct has no implicit padding: the packed words are its layout
FILM_GRAIN_TABLES_BYTES = _abi.define("SVTHIP_FILM_GRAIN_TABLES_BYTES")
FILM_GRAIN_NOISE_BLOCK_SIZE = _abi.define("SVTHIP_FILM_GRAIN_NOISE_BLOCK_SIZE")
FILM_GRAIN_NOISE_LAG = _abi.define("SVTHIP_FILM_GRAIN_NOISE_LAG")
FILM_GRAIN_NOISE_SHAPE_SQUARE = _abi.define("SVTHIP_FILM_GRAIN_NOISE_SHAPE_SQUARE")
FILM_GRAIN_NOISE_OK = _abi.define("SVTHIP_FILM_GRAIN_NOISE_OK")
FILM_GRAIN_NOISE_INSUFFICIENT_FLAT_BLOCKS = _abi.define("SVTHIP_FILM_GRAIN_NOISE_INSUFFICIENT_FLAT_BLOCKS")
FILM_GRAIN_NOISE_INTERNAL_ERROR = _abi.define("SVTHIP_FILM_GRAIN_NOISE_INTERNAL_ERROR")
FILM_GRAIN_FLAT_TABLES_DOUBLES = _abi.define("SVTHIP_FILM_GRAIN_FLAT_TABLES_DOUBLES")


def film_grain_wiener_workspace_bytes(width: int, height: int) -> int:
    """bytes of the three float planes svthip_film_grain_wiener_filter_dev writes and svthip_film_grain_dither_dev reads"""
    return int(lib().svthip_film_grain_wiener_workspace_bytes(width, height))


def film_grain_noise_psd_default(block_size: int, factor: float) -> float:
    """aom_noise_psd_get_default_value in float"""
    f, out = C.c_float(factor), C.c_float()
    _check(lib().svthip_film_grain_noise_psd_default(block_size, C.byref(f), C.byref(out)))
    return out.value


def film_grain_noise_state_dtype() -> np.dtype:
    """svthip_film_grain_noise_state: latest[3] and combined[3] of svthip_film_grain_noise_channel, status"""
    return _abi.dtype("svthip_film_grain_noise_state")


def film_grain_flat_block_features_dtype() -> np.dtype:
    """svthip_film_grain_flat_block_features: trace, ratio, norm, var of one 32x32 block"""
    return _abi.dtype("svthip_film_grain_flat_block_features")


def film_grain_param_offsets() -> dict:
    """{field: byte offset} of svthip_film_grain_params, random_seed and reserved included"""
    return {name: _LAYOUT.fields[name][1] for name in _LAYOUT.names}


def _flat(v):
    if isinstance(v, (list, tuple)):
        return [x for item in v for x in _flat(item)]
    return [int(v)]


def film_grain_params(**fields):
    """svthip_film_grain_params as a buffer the film-grain methods take: every field that is not named is 0; arrays may be shorter than
    the C array (the rest is 0) and scaling points are given as [[x, y], ...]"""
    unknown = set(fields) - set(_LAYOUT.names) | set(fields) & {"reserved"}
    if unknown:
        raise TypeError(f"svthip_film_grain_params has no field {sorted(unknown)}")
    words = []
    for name, _, n in _FILM_GRAIN_FIELDS:
        v = _flat(fields.get(name, 0))
        if len(v) > n:
            raise ValueError(f"{name} holds {n} values (got {len(v)})")
        words += v + [0] * (n - len(v))
    return C.create_string_buffer(struct.pack(_PACKED, *words), FILM_GRAIN_PARAMS_BYTES)


def _planes(ptrs, strides):
    return (C.c_void_p * 3)(*ptrs) if ptrs is not None else None, (C.c_uint32 * 3)(*strides) if strides is not None else None


class FilmGrain:
    """the film-grain entries as Context methods; planes are (Y, Cb, Cr) device pointers to sample (0, 0), strides in samples"""

    def film_grain_tables_dev(self, params, bit_depth, d_tables, stream=None):
        """the templates and scaling tables of `params` at 8 or 10 bits into d_tables (FILM_GRAIN_TABLES_BYTES of int16)"""
        _check(lib().svthip_film_grain_tables_dev(self._h, params, bit_depth, d_tables, stream))

    def add_film_grain_dev(self, params, d_src, src_stride, d_dst, dst_stride, width, height, d_tables=None, stream=None):
        """av1_add_film_grain on 8-bit planes, out of place; d_tables None builds the tables in context scratch first"""
        src, ss = _planes(d_src, src_stride)
        dst, ds = _planes(d_dst, dst_stride)
        _check(lib().svthip_av1_add_film_grain_dev(self._h, params, src, ss, dst, ds, width, height, d_tables, stream))

    def highbd_add_film_grain_dev(self, params, d_src, src_stride, d_dst, dst_stride, width, height, bit_depth, d_tables=None, stream=None):
        """av1_add_film_grain on 16-bit planes of 10-bit samples"""
        src, ss = _planes(d_src, src_stride)
        dst, ds = _planes(d_dst, dst_stride)
        _check(lib().svthip_av1_highbd_add_film_grain_dev(self._h, params, src, ss, dst, ds, width, height, bit_depth, d_tables, stream))

    def film_grain_noise_model_dev(self, d_data, d_denoised, stride, width, height, d_flat_blocks, d_state, block_size=FILM_GRAIN_NOISE_BLOCK_SIZE,
                                   lag=FILM_GRAIN_NOISE_LAG, shape=FILM_GRAIN_NOISE_SHAPE_SQUARE, stream=None):
        """aom_noise_model_init + aom_noise_model_update on 8-bit planes with the given flat-block map into *d_state"""
        data, st = _planes(d_data, stride)
        den, _ = _planes(d_denoised, None)
        _check(lib().svthip_film_grain_noise_model_dev(self._h, data, den, st, width, height, block_size, lag, shape, d_flat_blocks, d_state, stream))

    def highbd_film_grain_noise_model_dev(self, d_data, d_denoised, stride, width, height, bit_depth, d_flat_blocks, d_state,
                                          block_size=FILM_GRAIN_NOISE_BLOCK_SIZE, lag=FILM_GRAIN_NOISE_LAG, shape=FILM_GRAIN_NOISE_SHAPE_SQUARE, stream=None):
        """the same on 16-bit planes of 10-bit samples"""
        data, st = _planes(d_data, stride)
        den, _ = _planes(d_denoised, None)
        _check(lib().svthip_highbd_film_grain_noise_model_dev(self._h, data, den, st, width, height, bit_depth, block_size, lag, shape, d_flat_blocks,
                                                              d_state, stream))

    def film_grain_flat_block_tables_dev(self, d_tables, stream=None):
        """A | AtA_inv of aom_flat_block_finder_init into d_tables (FILM_GRAIN_FLAT_TABLES_DOUBLES doubles)"""
        _check(lib().svthip_film_grain_flat_block_tables_dev(self._h, d_tables, stream))

    def film_grain_flat_block_features_dev(self, d_luma, stride, width, height, d_features, d_is_flat, d_tables=None,
                                           block_size=FILM_GRAIN_NOISE_BLOCK_SIZE, stream=None):
        """the features and thresholded is_flat byte of every 32x32 block of an 8-bit luma plane; d_tables None builds the tables in scratch"""
        _check(lib().svthip_film_grain_flat_block_features_dev(self._h, d_luma, stride, width, height, block_size, d_tables, d_features, d_is_flat, stream))

    def highbd_film_grain_flat_block_features_dev(self, d_luma, stride, width, height, bit_depth, d_features, d_is_flat, d_tables=None,
                                                  block_size=FILM_GRAIN_NOISE_BLOCK_SIZE, stream=None):
        """the same on a 16-bit plane of 10-bit samples"""
        _check(lib().svthip_highbd_film_grain_flat_block_features_dev(self._h, d_luma, stride, width, height, bit_depth, block_size, d_tables, d_features,
                                                                     d_is_flat, stream))

    def film_grain_wiener_filter_dev(self, d_data, stride, width, height, d_noise_psd, d_planes, block_size=FILM_GRAIN_NOISE_BLOCK_SIZE, stream=None):
        """the FFT filter stage of aom_wiener_denoise_2d on 8-bit planes into the three float planes at d_planes"""
        data, st = _planes(d_data, stride)
        psd, _ = _planes(d_noise_psd, None)
        _check(lib().svthip_film_grain_wiener_filter_dev(self._h, data, st, width, height, block_size, psd, d_planes, stream))

    def highbd_film_grain_wiener_filter_dev(self, d_data, stride, width, height, bit_depth, d_noise_psd, d_planes, block_size=FILM_GRAIN_NOISE_BLOCK_SIZE,
                                            stream=None):
        """the same on 16-bit planes of 10-bit samples"""
        data, st = _planes(d_data, stride)
        psd, _ = _planes(d_noise_psd, None)
        _check(lib().svthip_highbd_film_grain_wiener_filter_dev(self._h, data, st, width, height, bit_depth, block_size, psd, d_planes, stream))

    def film_grain_dither_dev(self, d_planes, d_denoised, stride, width, height, block_size=FILM_GRAIN_NOISE_BLOCK_SIZE, stream=None):
        """dither_and_quantize_lowbd of the three float planes into 8-bit planes"""
        den, st = _planes(d_denoised, stride)
        _check(lib().svthip_film_grain_dither_dev(self._h, d_planes, den, st, width, height, block_size, stream))

    def highbd_film_grain_dither_dev(self, d_planes, d_denoised, stride, width, height, bit_depth, block_size=FILM_GRAIN_NOISE_BLOCK_SIZE, stream=None):
        """dither_and_quantize_highbd into 16-bit planes of 10-bit samples"""
        den, st = _planes(d_denoised, stride)
        _check(lib().svthip_highbd_film_grain_dither_dev(self._h, d_planes, den, st, width, height, bit_depth, block_size, stream))

    def film_grain_wiener_denoise_dev(self, d_data, data_stride, d_denoised, denoised_stride, width, height, d_noise_psd,
                                      block_size=FILM_GRAIN_NOISE_BLOCK_SIZE, stream=None):
        """aom_wiener_denoise_2d on 8-bit planes, the float planes in context scratch"""
        data, ds = _planes(d_data, data_stride)
        den, ns = _planes(d_denoised, denoised_stride)
        psd, _ = _planes(d_noise_psd, None)
        _check(lib().svthip_film_grain_wiener_denoise_dev(self._h, data, ds, den, ns, width, height, block_size, psd, stream))

    def highbd_film_grain_wiener_denoise_dev(self, d_data, data_stride, d_denoised, denoised_stride, width, height, bit_depth, d_noise_psd,
                                             block_size=FILM_GRAIN_NOISE_BLOCK_SIZE, stream=None):
        """the same on 16-bit planes of 10-bit samples"""
        data, ds = _planes(d_data, data_stride)
        den, ns = _planes(d_denoised, denoised_stride)
        psd, _ = _planes(d_noise_psd, None)
        _check(lib().svthip_highbd_film_grain_wiener_denoise_dev(self._h, data, ds, den, ns, width, height, bit_depth, block_size, psd, stream))
