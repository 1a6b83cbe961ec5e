"""IntegerLookup and StringLookup on the device hash table of K26 (csrc/vocab.hip): raw tokens -> the row numbers the
embedding kernels start from, with keras.layers.IntegerLookup / StringLookup's surface in output_mode "int".

Index layout (Keras'): [mask_token -> 0][num_oov_indices OOV slots][the vocabulary in order].  An OOV token goes to the
single OOV slot, or with several to floormod(token, num_oov_indices) from the first one; with num_oov_indices = 0 it is
an error (index -1 in a captured step, where the error word cannot be read).  `adapt` counts tokens on the device
(krs_vocab_upsert in ADD mode, growing the table by rehash) and orders them as Keras' finalize_state does: count
descending, ties by token descending, cut to max_tokens (which counts the mask and OOV entries)."""

from __future__ import annotations

import hashlib

import numpy as np
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import vocab_ops as V
from keras_rs_amd.layers import base
from keras_rs_amd.layers.embed_reduce import Ragged


def fingerprint(data: bytes) -> int:
    """The int64 a string's UTF-8 bytes stand for on the device: hashlib.blake2b with an 8-byte digest, read as a
    little-endian signed integer."""
    return int.from_bytes(hashlib.blake2b(data, digest_size=8).digest(), "little", signed=True)


def _is_scalar_token(x) -> bool:
    return isinstance(x, (int, str, bytes, np.integer, np.str_, np.bytes_))


class _Lookup(base.Layer):
    """What the two layers share: Keras' argument rules, the vocabulary with its special entries, the lazy device
    table, the call over tensors and Ragged, adapt and the state.  A subclass turns its tokens into int64 keys."""

    def __init__(self, max_tokens, num_oov_indices, mask_token, oov_token, vocabulary, output_mode, invert=False,
                 sparse=False, idf_weights=None, pad_to_max_tokens=False, **kwargs):
        super().__init__(**kwargs)
        if output_mode != "int":
            raise NotImplementedError(f"output_mode={output_mode!r} is not supported: K26 writes indices (\"int\")")
        if invert:
            raise NotImplementedError("invert=True is not supported: K26 maps tokens to indices only")
        if sparse:
            raise NotImplementedError("sparse=True is not supported: it belongs to the non-int output modes")
        if idf_weights is not None:
            raise NotImplementedError("idf_weights is not supported: it belongs to output_mode=\"tf_idf\"")
        if isinstance(vocabulary, (str, bytes)):
            raise NotImplementedError(f"vocabulary={vocabulary!r} as a file path is not supported: pass the tokens")
        if max_tokens is not None and int(max_tokens) <= 1:
            raise ValueError(f"If set, `max_tokens` must be greater than 1. Received: max_tokens={max_tokens}")
        if int(num_oov_indices) < 0:
            raise ValueError(f"`num_oov_indices` must be greater than or equal to 0. Received: {num_oov_indices}")
        self.max_tokens = None if max_tokens is None else int(max_tokens)
        self.num_oov_indices = int(num_oov_indices)
        self.mask_token, self.oov_token = mask_token, oov_token
        self.output_mode, self.pad_to_max_tokens = output_mode, bool(pad_to_max_tokens)
        self._table = None
        self.register_buffer("vocabulary", torch.zeros(0, dtype=torch.int64, device=self._device))
        if vocabulary is not None:
            self.set_vocabulary(vocabulary)

    # ---- what a subclass defines --------------------------------------------------------------------------------
    def _key_of(self, token) -> int:
        raise NotImplementedError

    def _keys_of(self, inputs) -> torch.Tensor:
        """inputs of any shape -> keys of that shape on the layer's device (int32 / int64)"""
        raise NotImplementedError

    def _set_tokens(self, tokens: list, keys: torch.Tensor) -> None:
        self.vocabulary = keys.to(device=self.vocabulary.device, dtype=torch.int64)
        self._table = None

    def _tokens(self) -> list:
        raise NotImplementedError

    # ---- Keras' vocabulary rules ----------------------------------------------------------------------------------
    def _token_start_index(self) -> int:
        return self.num_oov_indices + (0 if self.mask_token is None else 1)

    def _special_tokens(self) -> list:
        return ([] if self.mask_token is None else [self.mask_token]) + [self.oov_token] * self.num_oov_indices

    def set_vocabulary(self, vocabulary) -> None:
        if isinstance(vocabulary, torch.Tensor):
            vocabulary = vocabulary.detach().cpu().tolist()
        tokens = [t.item() if isinstance(t, np.generic) else t for t in np.asarray(vocabulary, dtype=object).reshape(-1)]
        special = self._special_tokens()
        if special and tokens[:len(special)] == special:      # a vocabulary saved with its special entries
            tokens = tokens[len(special):]
        for name, reserved in (("mask", self.mask_token), ("OOV", self.oov_token)):
            if reserved is not None and reserved in tokens:
                raise ValueError(f"Found reserved {name} token {reserved!r} at index {tokens.index(reserved)} of the "
                                 "vocabulary: reserved tokens may only lead it, in the order [mask, OOV...]")
        if len(set(tokens)) != len(tokens):
            raise ValueError("The passed vocabulary has at least one repeated term. Please uniquify your dataset.")
        if self.max_tokens is not None and len(tokens) + self._token_start_index() > self.max_tokens:
            raise ValueError(f"Attempted to set a vocabulary larger than the maximum vocab size. Received vocabulary "
                             f"size is {len(tokens) + self._token_start_index()}; `max_tokens` is {self.max_tokens}.")
        self._set_tokens(tokens, torch.tensor([self._key_of(t) for t in tokens], dtype=torch.int64))

    def get_vocabulary(self, include_special_tokens: bool = True) -> list:
        return (self._special_tokens() if include_special_tokens else []) + self._tokens()

    def vocabulary_size(self) -> int:
        return int(self.vocabulary.numel()) + self._token_start_index()

    # ---- the device table -----------------------------------------------------------------------------------------
    def table(self) -> V.Table:
        if self._table is None:
            self._table = V.build_table(self.vocabulary)
        return self._table

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._table = None      # (the vocabulary may have moved: the table is built again where it is now)
        return out

    def _indices(self, keys: torch.Tensor) -> torch.Tensor:
        mask = None if self.mask_token is None else self._key_of(self.mask_token)
        check = self.num_oov_indices == 0 and not base.stream_capturing()
        err = torch.zeros(1, dtype=torch.int32, device=keys.device) if check else None
        out = V.lookup(self.table(), keys, mask_token=mask, num_oov_indices=self.num_oov_indices, err_flag=err)
        if err is not None and int(err.item()) & L.FLAG_OOV_TOKEN:
            raise ValueError("found out-of-vocabulary tokens with `num_oov_indices=0`: set `num_oov_indices` to 1 or "
                             "more, or keep the inputs inside the vocabulary")
        return out

    def call(self, inputs):
        if isinstance(inputs, Ragged):
            return Ragged(self._indices(self._keys_of(inputs.values)), inputs.row_offsets)
        return self._indices(self._keys_of(inputs))

    # ---- adapt ----------------------------------------------------------------------------------------------------
    def adapt(self, data, steps: int | None = None) -> None:
        """Builds the vocabulary from a tensor (one batch) or an iterable of batches: counted on the device, ordered by
        count descending with ties by token descending, the mask token dropped, cut to max_tokens."""
        one = isinstance(data, (torch.Tensor, np.ndarray, Ragged)) or \
            (isinstance(data, (list, tuple)) and (len(data) == 0 or _is_scalar_token(data[0])))
        table = V.new_table(0, self.vocabulary.device)
        for i, batch in enumerate([data] if one else data):
            if steps is not None and i >= steps:
                break
            keys = self._keys_of(batch.values if isinstance(batch, Ragged) else batch)
            table = V.count_into(table, keys.to(torch.int64))
        keys, counts = V.export(table)
        if self.mask_token is not None:
            keep = keys != self._key_of(self.mask_token)
            keys, counts = keys[keep], counts[keep]
        room = None if self.max_tokens is None else self.max_tokens - self._token_start_index()
        self._finalize(keys, counts, room)

    def _finalize(self, keys, counts, room) -> None:
        raise NotImplementedError

    # ---- config and state -----------------------------------------------------------------------------------------
    def get_config(self) -> dict:
        cfg = super().get_config()
        cfg.update(max_tokens=self.max_tokens, num_oov_indices=self.num_oov_indices, mask_token=self.mask_token,
                   oov_token=self.oov_token, vocabulary=self._tokens() or None, output_mode=self.output_mode,
                   invert=False, sparse=False, idf_weights=None, pad_to_max_tokens=self.pad_to_max_tokens)
        return cfg

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        saved = state_dict.get(prefix + "vocabulary")
        if saved is not None:      # (any length: the buffer takes the saved shape and the table is built again)
            self.vocabulary = torch.empty_like(saved, device=self.vocabulary.device)
            self._table = None
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class IntegerLookup(_Lookup):
    """keras.layers.IntegerLookup in output_mode "int": int32 / int64 tokens of any shape (or a Ragged) -> int64
    indices.  Every int64 is a legal token.  state_dict holds the vocabulary tensor; the table is rebuilt on load."""

    def __init__(self, max_tokens=None, num_oov_indices=1, mask_token=None, oov_token=-1, vocabulary=None,
                 vocabulary_dtype="int64", idf_weights=None, invert=False, output_mode="int", sparse=False,
                 pad_to_max_tokens=False, **kwargs):
        if vocabulary_dtype not in ("int64", "int32"):
            raise ValueError(f"`vocabulary_dtype` must be 'int64' or 'int32'. Received: {vocabulary_dtype!r}")
        self.vocabulary_dtype = vocabulary_dtype
        super().__init__(max_tokens, num_oov_indices, mask_token, oov_token, vocabulary, output_mode, invert=invert,
                         sparse=sparse, idf_weights=idf_weights, pad_to_max_tokens=pad_to_max_tokens, **kwargs)

    def _key_of(self, token) -> int:
        return int(token)

    def _keys_of(self, inputs) -> torch.Tensor:
        t = inputs if isinstance(inputs, torch.Tensor) else torch.as_tensor(np.asarray(inputs))
        if t.dtype not in (torch.int32, torch.int64):
            t = t.to(torch.int64)
        return t.to(self.vocabulary.device)

    def _tokens(self) -> list:
        return self.vocabulary.cpu().tolist()

    def _finalize(self, keys, counts, room) -> None:
        order = torch.argsort(keys, descending=True, stable=True)
        order = order[torch.argsort(counts[order], descending=True, stable=True)]
        self._set_tokens([], keys[order][:room])

    def get_config(self) -> dict:
        return {**super().get_config(), "vocabulary_dtype": self.vocabulary_dtype}


class StringLookup(_Lookup):
    """keras.layers.StringLookup in output_mode "int" over the same device table.  Strings cannot live on the device:
    each string's UTF-8 bytes are fingerprinted on the host to an int64 with hashlib.blake2b(digest_size=8) (read
    little-endian, signed), and the fingerprints are the table's keys.  Two distinct vocabulary strings with one
    fingerprint are refused when the vocabulary is set.  With num_oov_indices > 1 an OOV string's slot is the floor
    modulus of its FINGERPRINT, not TensorFlow's FarmHash bucket: the OOV slot of a string differs from Keras'.
    Inputs are (nested) lists or numpy arrays of str / bytes, or a Ragged of them."""

    def __init__(self, max_tokens=None, num_oov_indices=1, mask_token=None, oov_token="[UNK]", vocabulary=None,
                 idf_weights=None, invert=False, output_mode="int", pad_to_max_tokens=False, sparse=False,
                 encoding="utf-8", **kwargs):
        self.encoding = encoding
        self._strings: list = []
        self._seen: dict = {}      # fingerprint -> string, of everything adapt has met
        self._recording = False
        super().__init__(max_tokens, num_oov_indices, mask_token, oov_token, vocabulary, output_mode, invert=invert,
                         sparse=sparse, idf_weights=idf_weights, pad_to_max_tokens=pad_to_max_tokens, **kwargs)

    def _key_of(self, token) -> int:
        return fingerprint(token if isinstance(token, bytes) else str(token).encode(self.encoding))

    def _keys_of(self, inputs) -> torch.Tensor:
        arr = np.asarray(inputs, dtype=object)
        one = self._counted_key if self._recording else self._key_of
        keys = np.fromiter((one(s) for s in arr.reshape(-1)), dtype=np.int64, count=arr.size)
        return torch.from_numpy(keys.reshape(arr.shape)).to(self.vocabulary.device)

    def _set_tokens(self, tokens: list, keys: torch.Tensor) -> None:
        if len(set(keys.tolist())) != len(tokens):
            raise ValueError("two distinct vocabulary strings share one 64-bit fingerprint: the device table cannot "
                             "tell them apart")
        self._strings = [t.decode(self.encoding) if isinstance(t, bytes) else str(t) for t in tokens]
        super()._set_tokens(tokens, keys)

    def _tokens(self) -> list:
        return list(self._strings)

    def adapt(self, data, steps: int | None = None) -> None:
        self._seen, self._recording = {}, True
        try:
            super().adapt(data, steps)
        finally:
            self._recording = False

    def _counted_key(self, s) -> int:
        s = s.decode(self.encoding) if isinstance(s, bytes) else str(s)
        key = self._key_of(s)
        if self._seen.setdefault(key, s) != s:
            raise ValueError(f"the strings {self._seen[key]!r} and {s!r} share one 64-bit fingerprint")
        return key

    def _finalize(self, keys, counts, room) -> None:      # (strings order on the host: the device holds fingerprints)
        pairs = sorted(((c, self._seen[k]) for k, c in zip(keys.cpu().tolist(), counts.cpu().tolist())), reverse=True)
        tokens = [s for _, s in pairs][:room]
        self._set_tokens(tokens, torch.tensor([self._key_of(t) for t in tokens], dtype=torch.int64))

    def get_config(self) -> dict:
        return {**super().get_config(), "encoding": self.encoding}

    def get_extra_state(self):
        return list(self._strings)

    def set_extra_state(self, state) -> None:
        self._strings = list(state)
