"""AV1 film-grain synthesis (svthip_film_grain_tables_dev, svthip_av1_[highbd_]add_film_grain_dev): pointer marshalling only.

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
