"""K26 on the host: the device hash table of csrc/vocab.hip behind plain functions -- build a vocabulary's table, look
ids up, count tokens into a table (growing it by rehash), export its (token, count) pairs.

A table is one int64 buffer on the device: 16 header words, then `slots` pairs {key, payload} (include/krs.h, K26).
Every argument is checked before the first launch.  There is no CPU fallback."""

from __future__ import annotations

import ctypes as C

import torch

from keras_rs_amd import _lib as L

_OUT_DTYPES = (torch.int32, torch.int64)


class Table:
    """buf: the device buffer; slots: its slot count; capacity: the tokens it may hold at load 0.5."""

    def __init__(self, buf: torch.Tensor, slots: int):
        self.buf, self.slots = buf, slots

    @property
    def capacity(self) -> int:
        return self.slots // 2

    def n_items(self) -> int:
        """The number of distinct tokens in the table (a host wait: the count is the header's first word)."""
        return int(self.buf[0].item())


def slots_for(n_tokens: int) -> int:
    size = int(L.lib().krs_vocab_table_bytes(int(n_tokens)))
    if size == 0:
        raise L.KrsError(f"vocab: cannot size a table for {n_tokens} tokens")
    return (size - 8 * L.VOCAB_HEADER_WORDS) // 16


def home_slot(key: int, slots: int) -> int:
    return int(L.lib().krs_vocab_home_slot(int(key), int(slots)))


def last_route() -> L.VocabRoute:
    route = L.VocabRoute()
    L.lib().krs_vocab_last_route(C.byref(route))
    return route


def _keys(t, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise L.KrsError(f"{what}: expected a device tensor, got {type(t).__name__}")
    L.require_device(t, what)
    L.itype(t)
    return t.detach().reshape(-1).contiguous()


def _upsert(table: Table, keys, payloads, mode: int, init: bool, err: torch.Tensor | None) -> None:
    n = 0 if keys is None else keys.numel()
    rc = L.lib().krs_vocab_upsert(L.ptr(table.buf), table.slots, L.ptr(keys), L.I64 if keys is None else L.itype(keys),
                                  L.ptr(payloads), n, mode, int(init), L.ptr(err), L.stream_ptr())
    L.check(rc, "krs_vocab_upsert")


def new_table(n_tokens: int, device, slots: int | None = None) -> Table:
    """An empty table with room for n_tokens at load 0.5 (or exactly `slots` slots, a multiple of 8)."""
    slots = slots_for(n_tokens) if slots is None else int(slots)
    if slots < 8 or slots % 8:
        raise L.KrsError(f"vocab: slots {slots} must be a multiple of 8, at least 8")
    if torch.device(device).type != "cuda":
        raise L.KrsError(f"vocab: a table lives on the GPU, not on {device} (no CPU fallback)")
    table = Table(torch.empty(L.VOCAB_HEADER_WORDS + 2 * slots, dtype=torch.int64, device=device), slots)
    _upsert(table, None, None, L.VOCAB_SET, True, None)
    return table


def build_table(vocab: torch.Tensor, slots: int | None = None) -> Table:
    """The table of a vocabulary [V] (int32 / int64, on the device): token vocab[i] -> i.  A repeated token is a
    ValueError, as in Keras (one host wait, at build time only)."""
    keys = _keys(vocab, "vocab build_table")
    if slots is not None and 2 * keys.numel() > int(slots):
        raise L.KrsError(f"vocab: {keys.numel()} tokens need {2 * keys.numel()} slots or more, got {slots}")
    table = new_table(keys.numel(), keys.device, slots)
    err = torch.zeros(1, dtype=torch.int32, device=keys.device)
    _upsert(table, keys, None, L.VOCAB_SET, False, err)
    flags = int(err.item())
    if flags & L.FLAG_DUPLICATE_TOKEN:
        raise ValueError("The passed vocabulary has at least one repeated term. Please uniquify your dataset.")
    if flags & L.FLAG_TABLE_FULL:
        raise L.KrsError("vocab build_table: the table overflowed")
    return table


def lookup(table: Table, ids: torch.Tensor, mask_token: int | None = None, num_oov_indices: int = 1,
           out_dtype: torch.dtype = torch.int64, err_flag: torch.Tensor | None = None, route_hint: int = L.VOCAB_AUTO,
           ids_per_lane: int = 0) -> torch.Tensor:
    """ids (any shape, int32 / int64) -> indices of the same shape under Keras' layout [mask][OOV][vocabulary].  With
    num_oov_indices == 0 an unknown token gives -1 and ORs FLAG_OOV_TOKEN into err_flag (int32 [1], optional).  No
    host wait: the call captures into a HIP graph."""
    if not isinstance(ids, torch.Tensor):
        raise L.KrsError(f"vocab lookup: expected a device tensor, got {type(ids).__name__}")
    L.require_device(ids, "vocab lookup ids")
    itype = L.itype(ids)
    if out_dtype not in _OUT_DTYPES:
        raise L.KrsError(f"vocab lookup: out_dtype {out_dtype} must be int32 or int64")
    if int(num_oov_indices) < 0:
        raise ValueError(f"`num_oov_indices` must be greater than or equal to 0. Received: {num_oov_indices}")
    if err_flag is not None and (err_flag.dtype != torch.int32 or err_flag.numel() != 1 or not err_flag.is_cuda):
        raise L.KrsError("vocab lookup: err_flag must be one int32 on the device")
    flat = ids.detach().reshape(-1)
    flat = flat if flat.is_contiguous() else flat.contiguous()
    out = torch.empty(flat.numel(), dtype=out_dtype, device=ids.device)
    rc = L.lib().krs_vocab_lookup(L.ptr(table.buf), table.slots, L.ptr(flat), itype, flat.numel(),
                                  int(mask_token is not None), 0 if mask_token is None else int(mask_token),
                                  int(num_oov_indices), L.ptr(out), L.I64 if out_dtype == torch.int64 else L.I32,
                                  L.ptr(err_flag), int(route_hint), int(ids_per_lane), L.stream_ptr())
    L.check(rc, "krs_vocab_lookup")
    return out.reshape(ids.shape)


def export(table: Table):
    """(keys [items], payloads [items]) of the occupied slots in slot order, the side slot last (one host wait)."""
    items = table.n_items()
    dev = table.buf.device
    keys = torch.empty(items, dtype=torch.int64, device=dev)
    payloads = torch.empty(items, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    size = int(L.lib().krs_vocab_export_workspace_bytes(table.slots))
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    rc = L.lib().krs_vocab_export(L.ptr(table.buf), table.slots, L.ptr(keys), L.ptr(payloads), items, L.ptr(count),
                                  L.ptr(ws), size, L.stream_ptr())
    L.check(rc, "krs_vocab_export")
    return keys, payloads


def count_into(table: Table, ids: torch.Tensor) -> Table:
    """Adds one to the count of every token of ids.  When the batch could push the load past 0.5 (every id a new
    token), the table first grows by rehash: its (token, count) pairs are upserted into one twice as large or larger.
    Returns the table to go on with."""
    keys = _keys(ids, "vocab count_into")
    if keys.numel() == 0:
        return table
    need = table.n_items() + keys.numel()
    if need > table.capacity:
        old_keys, old_counts = export(table)
        table = new_table(max(need, 2 * table.capacity), keys.device)
        if old_keys.numel():
            _upsert(table, old_keys, old_counts, L.VOCAB_ADD, False, None)
    _upsert(table, keys, None, L.VOCAB_ADD, False, None)
    return table
