"""Checkpoint loading and the per-process engine handle shared by the rankers.

Replaces `T5ForConditionalGeneration.from_pretrained(..., device_map='auto', torch_dtype=fp16)` of
ref: llmrankers/pointwise.py:20-24 and llmrankers/setwise.py:46-50: reads a HuggingFace-layout checkpoint
directory (config.json + *.safetensors), hands every tensor to the C ABI (rk_engine_load_tensor) and finalises
the MI355X engine.  No torch model is ever built and there is no CPU path: device='cpu' raises.
"""
from __future__ import annotations

import json
import os
from typing import Iterator, List, Sequence, Tuple

import numpy as np

from . import _synth
from ._engine import RkEngine, RkError, RkLlamaEngine


def parse_device(device) -> int:
    """'cuda' (the reference's default, ref: run.py:222), 'cuda:N', 'hip', 'hip:N' or an int -> ordinal."""
    if isinstance(device, int):
        return device
    s = str(device).lower()
    if s == "cpu":
        raise RuntimeError("the MI355X engine has no CPU path (device='cpu'); use the HuggingFace reference for CPU runs")
    if s in ("cuda", "hip", "gpu"):
        # one process per GPU under torchrun: 'cuda' means "this rank's GPU" (LOCAL_RANK), ordinal 0 otherwise
        return int(os.environ.get("LOCAL_RANK", "0") or 0)
    for pre in ("cuda:", "hip:"):
        if s.startswith(pre):
            return int(s[len(pre):])
    raise ValueError(f"unrecognised device {device!r}")


def resolve_checkpoint(model_name_or_path: str, cache_dir=None) -> str:
    """A local HuggingFace-layout directory, or a hub id ('google/flan-t5-large', as the reference's README and
    run.py use) resolved through huggingface_hub's cache (downloading when the machine is online) — the same lookup
    from_pretrained does (ref: pointwise.py:15-24)."""
    if os.path.isdir(model_name_or_path):
        return model_name_or_path
    try:
        from huggingface_hub import snapshot_download
        st = ["config.json", "*.safetensors", "*.safetensors.index.json"]
        pt = ["config.json", "pytorch_model*.bin", "pytorch_model.bin.index.json"]

        def has_weights(d):
            names = os.listdir(d)
            return any(n.endswith(".safetensors") or (n.startswith("pytorch_model") and n.endswith(".bin")) for n in names)
        # safetensors first; the .bin files only when the repository has none (hub models that ship both are not fetched
        # twice).  A cache hit that holds config.json but no weights falls through to the online download.
        for kw in ({"local_files_only": True}, {}):
            for patterns in (st, pt):
                try:
                    d = snapshot_download(model_name_or_path, cache_dir=cache_dir, allow_patterns=patterns, **kw)
                except Exception:
                    continue
                if has_weights(d):
                    return d
        raise FileNotFoundError("no weight files (model*.safetensors / pytorch_model*.bin) found locally or on the hub")
    except Exception as exc:
        raise FileNotFoundError(
            f"{model_name_or_path!r} is neither a local checkpoint directory nor a hub model reachable from here ({exc})") from None


def read_config(model_dir: str) -> dict:
    path = os.path.join(model_dir, "config.json")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not found: not a HuggingFace-layout checkpoint directory")
    with open(path) as f:
        return json.load(f)


def iter_checkpoint_tensors(model_dir: str) -> Iterator[Tuple[str, np.ndarray]]:
    """Yield (hf_name, ndarray) from model.safetensors or a sharded safetensors checkpoint."""
    from safetensors import safe_open
    idx = os.path.join(model_dir, "model.safetensors.index.json")
    if os.path.exists(idx):
        with open(idx) as f:
            files = sorted(set(json.load(f)["weight_map"].values()))
    elif os.path.exists(os.path.join(model_dir, "model.safetensors")):
        files = ["model.safetensors"]
    else:
        yield from _iter_torch_bin(model_dir)
        return
    for fn in files:
        path = os.path.join(model_dir, fn)
        try:
            with safe_open(path, framework="np") as f:
                for k in f.keys():
                    yield k, f.get_tensor(k)
        except TypeError:
            # bf16 has no numpy dtype: read through torch (plumbing only) and hand raw bf16 bits to the engine
            import torch
            with safe_open(path, framework="pt") as f:
                for k in f.keys():
                    t = f.get_tensor(k)
                    if t.dtype == torch.bfloat16:
                        yield k, t.view(torch.int16).numpy().view(np.uint16)
                    else:
                        yield k, t.float().numpy()


LORA_PROJECTIONS = _synth.LORA_TARGETS      # the seven plain projections of a decoder layer


def _read_adapter_tensors(adapter_dir: str) -> dict:
    st = os.path.join(adapter_dir, "adapter_model.safetensors")
    if os.path.exists(st):
        from safetensors import safe_open
        import torch
        out = {}
        with safe_open(st, framework="pt") as f:            # (through torch: adapters are often bf16, which numpy lacks)
            for k in f.keys():
                out[k] = f.get_tensor(k).float().numpy()
        return out
    pt = os.path.join(adapter_dir, "adapter_model.bin")
    if os.path.exists(pt):
        import torch
        return {k: t.float().numpy() for k, t in torch.load(pt, map_location="cpu", weights_only=True).items()}
    raise FileNotFoundError(f"no adapter_model.safetensors or adapter_model.bin in {adapter_dir}")


def merge_lora(tensors, adapter_dir: str) -> Iterator[Tuple[str, np.ndarray]]:
    """Wrap iter_checkpoint_tensors: every weight a PEFT LoRA adapter targets is yielded in fp32 as W + scale * B @ A (scale =
    lora_alpha / r, with use_rslora lora_alpha / sqrt(r)), everything else untouched.  The merge happens once, on the host, before
    rk_engine_load_tensor rounds to fp16 - the reference serves the adapter unmerged in half precision through vLLM (ref:
    llmrankers/setwise.py:450-454, 491-498): a documented deviation ("Qwen2 family and Rank-R1").  Adapter keys are
    base_model.model.<hf name minus .weight>.lora_A.weight [r, in] and .lora_B.weight [out, r]; a key that matches no
    checkpoint tensor is an error, and so is anything but plain LoRA on the seven projections the engine holds."""
    with open(os.path.join(adapter_dir, "adapter_config.json")) as f:
        ac = json.load(f)
    if ac.get("peft_type", "LORA") != "LORA":
        raise NotImplementedError(f"adapter type {ac.get('peft_type')!r} is not supported by the MI355X engine (LoRA is)")
    if ac.get("use_dora"):
        raise NotImplementedError("DoRA adapters (use_dora) are not supported by the MI355X engine")
    if ac.get("bias", "none") != "none":
        raise NotImplementedError(f"LoRA adapters that train biases (bias={ac['bias']!r}) are not supported by the MI355X engine")
    if ac.get("modules_to_save"):
        raise NotImplementedError(f"LoRA adapters with modules_to_save ({ac['modules_to_save']}) are not supported by the MI355X engine")
    targets = ac.get("target_modules")
    if not isinstance(targets, (list, tuple)):
        raise NotImplementedError(f"target_modules must be a list of module names (got {targets!r})")
    bad = [m for m in targets if m.split(".")[-1] not in LORA_PROJECTIONS]
    if bad:
        raise NotImplementedError(f"LoRA on {bad} is not supported: the MI355X engine holds {LORA_PROJECTIONS} as plain projections")
    r, alpha = int(ac["r"]), float(ac["lora_alpha"])
    if ac.get("rank_pattern") or ac.get("alpha_pattern"):
        raise NotImplementedError("per-module LoRA ranks / alphas (rank_pattern, alpha_pattern) are not supported by the MI355X engine")
    scale = alpha / np.sqrt(r) if ac.get("use_rslora") else alpha / r
    pairs = {}
    for k, v in _read_adapter_tensors(adapter_dir).items():
        for tag in (".lora_A.weight", ".lora_B.weight"):
            if k.endswith(tag) and k.startswith("base_model.model."):
                name = k[len("base_model.model."):-len(tag)]
                if name.split(".")[-1] not in LORA_PROJECTIONS:
                    raise NotImplementedError(f"adapter tensor {k}: not one of the projections the MI355X engine holds")
                pairs.setdefault(name + ".weight", {})[tag[6]] = np.asarray(v, dtype=np.float32)
                break
        else:
            raise NotImplementedError(f"adapter tensor {k} is not a plain LoRA A / B matrix")
    for name, arr in tensors:
        ab = pairs.pop(name, None)
        if ab is None:
            yield name, arr
            continue
        if set(ab) != {"A", "B"}:
            raise ValueError(f"adapter for {name}: lora_A / lora_B incomplete")
        if arr.dtype == np.uint16:                              # raw bf16 bits (iter_checkpoint_tensors)
            arr = (arr.astype(np.uint32) << 16).view(np.float32)
        w = np.asarray(arr, dtype=np.float32)
        a, b = ab["A"], ab["B"]
        if a.shape != (r, w.shape[1]) or b.shape != (w.shape[0], r):
            raise ValueError(f"adapter for {name}: A {a.shape} / B {b.shape} do not fit the weight {w.shape} at rank {r}")
        yield name, (w + np.float32(scale) * (b @ a)).astype(np.float32)
    if pairs:
        raise KeyError(f"adapter tensors match no checkpoint tensor: {sorted(pairs)[:4]}{' ...' if len(pairs) > 4 else ''}")


def _iter_torch_bin(model_dir: str) -> Iterator[Tuple[str, np.ndarray]]:
    """pytorch_model.bin checkpoints (e.g. castorini/monot5-*): read with torch.load — loader plumbing only."""
    import torch
    idx = os.path.join(model_dir, "pytorch_model.bin.index.json")
    if os.path.exists(idx):
        with open(idx) as f:
            files = sorted(set(json.load(f)["weight_map"].values()))
    elif os.path.exists(os.path.join(model_dir, "pytorch_model.bin")):
        files = ["pytorch_model.bin"]
    else:
        raise FileNotFoundError(f"no model.safetensors[.index.json] or pytorch_model.bin[.index.json] in {model_dir}")
    for fn in files:
        sd = torch.load(os.path.join(model_dir, fn), map_location="cpu", weights_only=True)
        for k, t in sd.items():
            if t.dtype == torch.bfloat16:
                yield k, t.contiguous().view(torch.int16).numpy().view(np.uint16)
            elif t.dtype == torch.float16:
                yield k, t.numpy()
            else:
                yield k, t.float().numpy()


def require_decoder_positions(runtime, who: str) -> None:
    """Rankers that score or decode beyond ONE decoder position (qlm, setwise, listwise, PRP) call this when they are built: a
    T5 with 128-wide heads (t5-3b / t5-11b: monoT5-3B, duoT5-3B) runs on the engine at one position only, and none of the public
    checkpoints of that width is an instruction model such rankers could use."""
    if getattr(runtime, "one_position_only", False):
        raise NotImplementedError(f"{who} needs more than one decoder position; a T5 with d_kv=128 is served at one position only "
                                  "(MonoT5LlmRanker, PointwiseLlmRanker(method='yes_no'), DuoT5LlmRanker)")


class T5Runtime:
    """Engine + chunking so a call may exceed the engine's token capacity (results are batch-independent)."""

    @property
    def one_position_only(self) -> bool:
        """The model has 128-wide heads: the engine serves score() with a one-token decoder prefix and compare_pairs() only."""
        return int(self.dims.d_kv) == 128

    def _served(self, call, *args):
        """An engine call; the engine's refusal of an entry point a 128-wide model does not have -> NotImplementedError with its message."""
        try:
            return call(*args)
        except RkError as err:
            if self.one_position_only and "d_kv=128" in str(err):
                raise NotImplementedError(str(err)) from None
            raise

    def __init__(self, model_name_or_path: str, device, max_tokens: int = 49152, max_seqs: int = 256,
                 max_dec_len: int = 136, cache_dir=None):
        model_name_or_path = resolve_checkpoint(model_name_or_path, cache_dir)
        cfg = read_config(model_name_or_path)
        self.model_type = cfg.get("model_type")
        if self.model_type != "t5":
            raise NotImplementedError(f"Model type {self.model_type} is not supported yet by the MI355X engine")
        self.config = cfg
        self.dims = _synth.T5Dims.from_hf_config(cfg)
        self.decoder_start_token_id = cfg.get("decoder_start_token_id", 0)
        self.max_tokens, self.max_seqs = max_tokens, max_seqs
        self.engine = RkEngine(self.dims, parse_device(device), max_tokens, max_seqs, max_dec_len)
        self.engine.load_state(iter_checkpoint_tensors(model_name_or_path))

    @classmethod
    def from_engine(cls, engine: RkEngine, dims=None) -> "T5Runtime":
        """Wrap an engine that is already loaded (bench.py, tools/): no checkpoint directory involved."""
        self = cls.__new__(cls)
        self.dims = dims if dims is not None else engine.dims
        self.config, self.model_type, self.decoder_start_token_id = self.dims.to_hf_config(), "t5", 0
        self.max_tokens, self.max_seqs = int(engine.desc.max_tokens), int(engine.desc.max_seqs)
        self.engine = engine
        return self

    # -- multi-GPU: scores are collected by the engine's own RCCL communicator (rk_comm_*) --------------------
    COMM_FLOATS_PER_RANK = 65536      # send-buffer capacity (256 KB per rank): hits / world x outputs per passage

    def comm_ready(self) -> bool:
        """an engine communicator exists (any world size: one rank gathers with itself over the same calls)"""
        return self.comm_capacity > 0

    def comm_rank_world(self):
        """(rank, world) of the engine communicator"""
        return int(getattr(self.engine, "comm_rank", 0)), int(getattr(self.engine, "comm_world", 1))

    def comm_init_from_process_group(self, max_floats_per_rank: int = 0):
        """One process per GPU under torchrun: take rank / world from the initialised torch.distributed group, use it
        ONLY to hand rank 0's RCCL id to the other ranks, and build the engine's communicator (collective)."""
        import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()
        ids = [self.engine.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(ids, src=0)
        self.engine.comm_init(ids[0], rank, world, max_floats_per_rank or self.COMM_FLOATS_PER_RANK)

    @property
    def comm_capacity(self) -> int:
        """Floats per rank the live communicator can ship - the ENGINE's figure, whoever built the communicator (this
        runtime, bench.py or a tool through engine.comm_init): one value for the check and the message on every rank."""
        return int(getattr(self.engine, "comm_capacity", 0) or 0)

    def ensure_comm(self) -> bool:
        """Called by a candidate-sharding ranker before its first sharded query: under an initialised process group of
        more than one rank the engine communicator is built once (every rank gets here - the call is collective).
        Returns comm_ready().  A failure to bring RCCL up raises: there is no silent host-side substitute on a GPU run."""
        if self.comm_ready():
            return True
        try:
            import torch.distributed as dist
        except Exception:
            return False
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return False
        self.comm_init_from_process_group()
        return self.comm_ready()

    def sharded_scores(self, kind: str, seqs, arg, out_ids, width_floats: int, tail=None, tail_offset: int = 0):
        """This rank's share of one query -> (local raw outputs, allv [world, width_floats]) with ONE RCCL all_gather.
        The share may take several engine calls (more than max_seqs sequences / max_tokens tokens): each call's scores are
        appended to the engine's send buffer on the device (rk_comm_append_scores_slot), then the whole share is shipped.
        Every rank issues exactly one collective per query whatever its chunk count (also with an empty share).
        `tail`: host floats that travel in the same gather at `tail_offset` of this rank's row (the per-passage token counts
        behind the reference's counters).  width_floats is the same on every rank (it follows from the candidate count and
        the world size alone), so the capacity check below fails on ALL ranks or none - never inside the collective."""
        if width_floats > self.comm_capacity:
            raise ValueError(f"{width_floats} floats per rank exceed the communicator's send buffer ({self.comm_capacity}); "
                             "build it with comm_init_from_process_group(max_floats_per_rank=...)")
        k = len(out_ids) if kind == "score" else 1
        if tail is not None and len(tail):
            self.engine.comm_append_host(np.asarray(tail, dtype=np.float32), tail_offset)
        parts, off, done = [], 0, 0
        for chunk in self._chunks(seqs):
            if kind == "qlm_many":                               # arg = one label sequence per sequence (several queries' shares)
                part = self.engine.qlm_many(chunk, arg[done:done + len(chunk)])
            else:
                part = self.engine.qlm(chunk, arg) if kind == "qlm" else self.engine.score(chunk, arg, out_ids)
            done += len(chunk)
            n = len(chunk) * k
            self.engine.comm_append(n, off, slot=0)              # blocking calls leave their scores in slot 0
            parts.append(np.asarray(part, dtype=np.float32).reshape(-1))
            off += n
        local = np.concatenate(parts) if parts else np.zeros(0, np.float32)
        return local, self.engine.comm_all_gather_appended(width_floats)

    def all_gather_last_scores(self, n_floats: int) -> np.ndarray:
        """[world, n_floats]: the first n_floats of slot 0's device score buffer of every rank (one RCCL all_gather; a
        share that fits ONE engine call - bench.py's grouped launches; rankers use sharded_scores)."""
        self.engine.comm_all_gather(n_floats, slot=0)
        return self.engine.comm_read_gathered(0)

    def _chunks(self, seqs: Sequence[Sequence[int]]) -> Iterator[List[Sequence[int]]]:
        cur, tok = [], 0
        for s in seqs:
            if len(s) > self.max_tokens:
                raise ValueError(f"a prompt of {len(s)} tokens exceeds the engine capacity {self.max_tokens}")
            if cur and (tok + len(s) > self.max_tokens or len(cur) == self.max_seqs):
                yield cur
                cur, tok = [], 0
            cur.append(s)
            tok += len(s)
        if cur:
            yield cur

    def score(self, seqs, dec_prefix, out_ids) -> np.ndarray:
        return np.concatenate([self._served(self.engine.score, c, dec_prefix, out_ids) for c in self._chunks(seqs)], axis=0)

    def score_stream(self, groups, dec_prefix, out_ids) -> np.ndarray:
        """Scores [n, len(out_ids)] of the token sequences that the iterable `groups` yields (lists of sequences, e.g. one
        query's prompts at a time), in order.  `groups` is consumed LAZILY: as soon as the sequences pulled so far fill an
        engine call (max_seqs / max_tokens - the same greedy cut as _chunks over the flat list) the call is staged and
        enqueued on the next batch slot, and the host goes on pulling - i.e. tokenising - the following sequences while the
        GPU works (rk_t5_stage_slot / rk_t5_score_slot return at once; only reading a slot's scores waits).  A call of six
        queries thus leaves the tokenisation of the first launch sequence exposed instead of all of it.  Same bits as
        score() on the flat list: a sequence's scores do not depend on what shares its call."""
        eng = self.engine
        n_slots = eng.num_slots
        parts, pending = [], []                                         # slots in submission order
        launched = 0
        cur, tok = [], 0

        def launch(chunk):
            nonlocal launched
            slot = launched % n_slots
            if len(pending) == n_slots:                                # the slot we are about to reuse must be drained
                parts.append(eng.read_scores(pending.pop(0)))
            eng.stage(chunk, slot=slot)
            eng.score_staged(dec_prefix, out_ids, slot=slot)
            pending.append(slot)
            launched += 1

        try:
            for group in groups:
                for s in group:
                    if len(s) > self.max_tokens:
                        raise ValueError(f"a prompt of {len(s)} tokens exceeds the engine capacity {self.max_tokens}")
                    if cur and (tok + len(s) > self.max_tokens or len(cur) == self.max_seqs):
                        launch(cur)
                        cur, tok = [], 0
                    cur.append(s)
                    tok += len(s)
            if cur:
                launch(cur)
        finally:
            # whatever happened above (a prompt too long, the caller's generator raising): no slot stays in flight
            for s0 in pending:
                parts.append(eng.read_scores(s0))
        return np.concatenate(parts, axis=0) if parts else np.zeros((0, len(out_ids)), np.float32)

    def score_batches(self, batches, dec_prefix, out_ids) -> List[np.ndarray]:
        """Score several independent batches, keeping the engine's batch slots full: batch i+1 is staged and its
        encoder enqueued while the decoder chain of batch i still runs (rk_t5_stage_slot / rk_t5_score_slot).
        Results are identical to calling score() per batch; only the waiting is overlapped."""
        # The reference's batch_size only shapes its host loop; results do not depend on batch composition (ragged
        # execution), so consecutive batches are merged up to the engine's capacity: one launch sequence then covers
        # ~one query's candidates - better GEMM tile quantisation and ONE decoder chain instead of one per batch.
        batches = list(batches)
        allsc = self.score_stream(batches, dec_prefix, out_ids)
        out, pos = [], 0
        for b in batches:
            out.append(allsc[pos:pos + len(b)])
            pos += len(b)
        return out

    def score_async(self, seqs, dec_prefix, out_ids, slot: int):
        """Enqueue ONE engine call for `seqs` on batch slot `slot` and return at once -> a handle for score_collect, or None
        when the sequences do not fit one call (the caller then uses score(), which cuts them).  The caller owns the slot
        until it has collected: nothing else may be launched on it, and no blocking call may run, in between."""
        if not (0 < len(seqs) <= self.max_seqs and sum(len(s) for s in seqs) <= self.max_tokens):
            return None
        self.engine.stage(seqs, slot=slot)
        self.engine.score_staged(dec_prefix, out_ids, slot=slot)
        return slot

    def score_collect(self, handle) -> np.ndarray:
        """[n, len(out_ids)] scores of the call score_async enqueued (waits for it)."""
        return self.engine.read_scores(handle)

    # -- the duoT5 compare: pairs of sequences (the A/B and the B/A prompt), softmax and verdict on the device -----------------
    supports_compare_pairs = True

    def _pair_chunks(self, seqs) -> Iterator[List[Sequence[int]]]:
        """`_chunks` with a PAIR as the unit: the same greedy cut by max_seqs / max_tokens, never between the two orderings."""
        if len(seqs) % 2:
            raise ValueError(f"a compare needs pairs of sequences (got {len(seqs)})")
        if self.max_seqs < 2:
            raise ValueError(f"a pair of prompts exceeds the engine capacity of {self.max_seqs} sequence")
        cur, tok = [], 0
        for p in range(0, len(seqs), 2):
            n = len(seqs[p]) + len(seqs[p + 1])
            if n > self.max_tokens:
                raise ValueError(f"a pair of prompts of {n} tokens exceeds the engine capacity {self.max_tokens}")
            if cur and (tok + n > self.max_tokens or len(cur) + 2 > self.max_seqs):
                yield cur
                cur, tok = [], 0
            cur += [seqs[p], seqs[p + 1]]
            tok += n
        if cur:
            yield cur

    def compare_pairs(self, seqs, dec_start, false_id, true_id):
        """(logits [2n, 2], p_true [2n], first_wins [n] bool) of the n pairs (seqs[2p], seqs[2p + 1]): RkEngine.compare_pairs, cut
        into engine calls of whole pairs.  A pair's figures do not depend on what shares its call."""
        parts = [self.engine.compare_pairs(c, dec_start, false_id, true_id) for c in self._pair_chunks(seqs)]
        if not parts:
            return np.zeros((0, 2), np.float32), np.zeros(0, np.float32), np.zeros(0, bool)
        return tuple(np.concatenate([p[i] for p in parts], axis=0) for i in range(3))

    def compare_async(self, seqs, dec_start, false_id, true_id, slot: int):
        """score_async's twin: ONE compare call for the pairs in `seqs` enqueued on batch slot `slot` -> a handle for
        compare_collect, or None when they do not fit one call (the caller then uses compare_pairs, which cuts them)."""
        if not (0 < len(seqs) <= self.max_seqs and len(seqs) % 2 == 0 and sum(len(s) for s in seqs) <= self.max_tokens):
            return None
        self.engine.stage(seqs, slot=slot)
        self.engine.compare_staged(dec_start, false_id, true_id, slot=slot)
        return slot

    def compare_collect(self, handle):
        """compare_pairs' triple of the call compare_async enqueued (waits for it)."""
        return self.engine.read_scores(handle)

    def qlm(self, seqs, labels) -> np.ndarray:
        return np.concatenate([self._served(self.engine.qlm, c, labels) for c in self._chunks(seqs)], axis=0)

    def qlm_many(self, seqs, labels_per_seq) -> np.ndarray:
        """qlm scores of sequences with their OWN labels each (the passages of several queries): one engine call per capacity
        chunk, whatever the number of queries in it.  Element b is bit for bit what qlm gives seqs[b] with labels_per_seq[b]."""
        parts, done = [], 0
        for c in self._chunks(seqs):
            parts.append(self._served(self.engine.qlm_many, c, labels_per_seq[done:done + len(c)]))
            done += len(c)
        return np.concatenate(parts, axis=0) if parts else np.zeros(0, np.float32)

    def qlm_batches(self, batches, labels) -> List[np.ndarray]:
        """qlm scores of several batches of ONE query (same labels): the reference's batch_size only shapes its host loop and a
        passage's score does not depend on what shares its call, so the batches go to the engine merged up to its capacity -
        one encoder / decoder / head sequence over the query's candidates instead of one per batch of 32."""
        batches = list(batches)
        allsc = self.qlm([s for b in batches for s in b], labels) if batches else np.zeros(0, np.float32)
        out, pos = [], 0
        for b in batches:
            out.append(allsc[pos:pos + len(b)])
            pos += len(b)
        return out

    supports_greedy_candidates = True

    def greedy(self, seqs, dec_prefix, max_new, eos_id=1, pad_id=0, candidates=None) -> np.ndarray:
        """[B, max_new] new tokens; columns after the step at which every row had finished hold -1.  `candidates`: see
        RkEngine.greedy (a hint that never changes the result)."""
        parts = []
        for c in self._chunks(seqs):
            toks, steps = self._served(self.engine.greedy, c, dec_prefix, max_new, eos_id, pad_id, candidates)
            toks = toks.copy()
            toks[:, steps:] = -1
            parts.append(toks)
        return np.concatenate(parts, axis=0)


    def generate(self, seqs, dec_prefix, max_new, eos_id=1, pad_id=0) -> np.ndarray:
        """`greedy`'s result ([B, max_new], -1 after the step at which every row of an engine call had finished) from the
        KV-cached incremental decoder (RkEngine.generate); chunked by capacity the same way."""
        parts = []
        for c in self._chunks(seqs):
            toks, steps = self._served(self.engine.generate, c, dec_prefix, max_new, eos_id, pad_id)
            toks = toks.copy()
            toks[:, steps:] = -1
            parts.append(toks)
        return np.concatenate(parts, axis=0)

def read_generation_settings(model_dir, cfg: dict) -> dict:
    """What the reference's bare `self.llm.generate(input_ids)` (ref: llmrankers/listwise.py:268) takes from the checkpoint:
    generation_config.json over config.json for eos_token_id (int or list -> list), pad_token_id (absent: the first EOS id, as
    HF's generate does), max_new_tokens, max_length, do_sample, and the sampling parameters temperature, top_k, top_p (absent:
    the defaults of HF's GenerationConfig, 1.0 / 50 / 1.0)."""
    gc = {}
    if model_dir and os.path.exists(os.path.join(model_dir, "generation_config.json")):
        with open(os.path.join(model_dir, "generation_config.json")) as f:
            gc = json.load(f)

    def pick(key):
        return gc[key] if gc.get(key) is not None else cfg.get(key)
    eos = pick("eos_token_id")
    eos = [] if eos is None else ([int(t) for t in eos] if isinstance(eos, (list, tuple)) else [int(eos)])
    pad = pick("pad_token_id")
    return {"eos_token_ids": eos, "pad_token_id": int(pad) if pad is not None else (eos[0] if eos else 0),
            "max_new_tokens": gc.get("max_new_tokens"), "max_length": gc.get("max_length"), "do_sample": bool(gc.get("do_sample")),
            "temperature": float(gc["temperature"]) if gc.get("temperature") is not None else 1.0,
            "top_k": int(gc["top_k"]) if gc.get("top_k") is not None else 50,
            "top_p": float(gc["top_p"]) if gc.get("top_p") is not None else 1.0}


def sampling_plan(runtime):
    """None for a checkpoint that decodes greedily (no do_sample: true in its generation settings), else (temperature, top_k,
    top_p) as HF's generate would apply them: the arguments of `set_sampling`.  For any runtime with a `generation` dict; a dict
    built by hand may lack the three keys (HF's defaults then)."""
    g = runtime.generation
    if not g.get("do_sample"):
        return None
    return float(g.get("temperature", 1.0)), int(g.get("top_k", 50)), float(g.get("top_p", 1.0))


def default_generation_length():
    """(max_new_tokens, max_length) of a bare `generate(input_ids)` when the checkpoint sets no length - resolve_max_new's logic
    (listwise.py) for a decoder-only prompt: transformers >= 5 has no default max_length and generates 20 new tokens; before,
    max_length = 20 counted the prompt."""
    try:
        from transformers import GenerationConfig
        ml = GenerationConfig().max_length
    except Exception:                      # (no transformers: the current default)
        ml = None
    return (20, None) if ml is None else (None, int(ml))


def hf_prompt_too_long_error():
    """the exception type HF's generate raises for a prompt that already reaches max_length (ValueError in transformers 4 and 5)"""
    return ValueError


WEIGHT_DTYPES = ("fp16", "fp8")


def refuse_t5_weight_dtype(weight_dtype):
    """The rankers' weight_dtype on a T5 checkpoint: "fp16" is what T5 runs; FP8 step weights exist for the Llama family only."""
    if weight_dtype not in WEIGHT_DTYPES:
        raise ValueError(f"weight_dtype must be one of {WEIGHT_DTYPES} (got {weight_dtype!r})")
    if weight_dtype != "fp16":
        raise NotImplementedError(f"weight_dtype={weight_dtype!r} is not supported for T5 checkpoints: FP8 step weights serve the Llama "
                                  "family's decoding step (weight_dtype='fp16' is what the T5 engine runs)")


def weight_dtype_kw(weight_dtype) -> dict:
    """The keyword a ranker adds to its runtime call: none for the default (the calls of a default ranker stay what they were)."""
    if weight_dtype not in WEIGHT_DTYPES:
        raise ValueError(f"weight_dtype must be one of {WEIGHT_DTYPES} (got {weight_dtype!r})")
    return {} if weight_dtype == "fp16" else {"weight_dtype": weight_dtype}


KV_DTYPES = ("fp16", "fp8")


def kv_dtype_kw(kv_dtype) -> dict:
    """The keyword a ranker adds to its runtime call: none for the default (the calls of a default ranker stay what they were)."""
    if kv_dtype not in KV_DTYPES:
        raise ValueError(f"kv_dtype must be one of {KV_DTYPES} (got {kv_dtype!r})")
    return {} if kv_dtype == "fp16" else {"kv_dtype": kv_dtype}


def refuse_t5_kv_dtype(kv_dtype):
    """The rankers' kv_dtype on a T5 checkpoint: "fp16" is what T5 runs; the FP8 K / V cache exists for the Llama family only."""
    if kv_dtype not in KV_DTYPES:
        raise ValueError(f"kv_dtype must be one of {KV_DTYPES} (got {kv_dtype!r})")
    if kv_dtype != "fp16":
        raise NotImplementedError(f"kv_dtype={kv_dtype!r} is not supported for T5 checkpoints: the FP8 K / V cache serves the Llama "
                                  "family's decoding step (kv_dtype='fp16' is what the T5 engine runs)")


_KV_DTYPE_CLASSES = {}          # (class, kv_dtype) -> the subclass class_with_kv_dtype hands out


def class_with_kv_dtype(cls, kv_dtype):
    """A ranker class whose runtime keeps an FP8 K / V cache (LlamaRuntime's kv_dtype; lossy, opt-in).  The rankers' constructors keep
    their parameter lists, so the option is the class's, like with_weight_dtype: Cls.with_kv_dtype("fp8")(model, ...)."""
    kv_dtype_kw(kv_dtype)                                              # ValueError for anything but "fp16" / "fp8"
    if kv_dtype == cls.kv_dtype:
        return cls
    if (cls, kv_dtype) not in _KV_DTYPE_CLASSES:                       # one subclass per (class, dtype), not one per call
        _KV_DTYPE_CLASSES[cls, kv_dtype] = type(cls.__name__, (cls,), {"kv_dtype": kv_dtype})
    return _KV_DTYPE_CLASSES[cls, kv_dtype]


MAX_DRAFT_TOKENS = 7


def draft_tokens_kw(draft_tokens) -> dict:
    """The keyword a caller adds to open_pool: none for 0 (the calls of a default ranker stay what they were)."""
    try:
        n = int(draft_tokens)
    except (TypeError, ValueError):
        n = -1
    if n != draft_tokens or not 0 <= n <= MAX_DRAFT_TOKENS:
        raise ValueError(f"draft_tokens must be an integer in 0..{MAX_DRAFT_TOKENS} (got {draft_tokens!r})")
    return {} if n == 0 else {"draft_tokens": n}


def generate_drafted(runtime, seqs, max_new, eos_ids, pad_id, draft_tokens) -> np.ndarray:
    """`runtime.generate`'s [B, max_new] rows (-1 behind a row's last token) decoded through a drafting pool of as many slots as there
    are prompts (one prompt: ONE slot, where the step has the most room for draft rows).  The tokens are generate's by the
    session's contract; only the number of steps differs."""
    kw = draft_tokens_kw(draft_tokens)
    n_slots = max(1, min(len(seqs), int(runtime.max_seqs) // (int(draft_tokens) + 1)))
    out = np.full((len(seqs), int(max_new)), -1, dtype=np.int32)
    with runtime.open_pool(max_new_cap=int(max_new), eos_ids=list(eos_ids), pad_id=int(pad_id), n_slots=n_slots, **kw) as pool:
        for b, ids in enumerate(seqs):
            pool.submit(b, ids, max_new)
        while pool.pending():
            for b, tokens in pool.wait():
                out[b, :len(tokens)] = tokens
    return out


class LlamaRuntime:
    """Decoder-only (Llama family) counterpart of T5Runtime: checkpoint directory -> rk_llama_* engine.  Replaces
    `AutoModelForCausalLM.from_pretrained(..., device_map='auto', torch_dtype=fp16)` of ref: llmrankers/setwise.py:65-69."""

    def __init__(self, model_name_or_path: str, device, max_tokens: int = 32768, max_seqs: int = 16, cache_dir=None,
                 accept_model_types=("llama",), adapter_dir=None, kv_dtype="fp16", weight_dtype="fp16"):
        """accept_model_types: the config.model_type values the caller serves - the reference's setwise / pairwise / listwise
        rankers refuse Qwen (ref: setwise.py:71), its Rank-R1 ranker runs on it.  adapter_dir: a PEFT LoRA adapter merged into
        the weights on the way in (merge_lora).  weight_dtype: "fp16", or "fp8" - FP8 step weights (RkLlamaEngine(weight_fp8=True):
        opt-in and lossy, one e4m3 rounding per weight of the projections the decoding step streams, behind the LoRA merge).
        kv_dtype: "fp16", or "fp8" - the decoding step's K / V cache in FP8 (RkLlamaEngine(kv_fp8=True): opt-in and lossy, one e4m3
        rounding per cached key and value element; head_dim 128 only).  The two combine freely."""
        if weight_dtype not in WEIGHT_DTYPES:
            raise ValueError(f"weight_dtype must be one of {WEIGHT_DTYPES} (got {weight_dtype!r})")
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"kv_dtype must be one of {KV_DTYPES} (got {kv_dtype!r})")
        self.weight_dtype, self.kv_dtype = weight_dtype, kv_dtype
        model_name_or_path = resolve_checkpoint(model_name_or_path, cache_dir)
        cfg = read_config(model_name_or_path)
        self.model_type = cfg.get("model_type")
        if self.model_type not in accept_model_types:
            raise NotImplementedError(f"Model type {self.model_type} is not supported yet by the MI355X engine")
        self.config = cfg
        self.dims = _synth.LlamaDims.from_hf_config(cfg)
        self.max_tokens, self.max_seqs = max_tokens, max_seqs
        self.generation = read_generation_settings(model_name_or_path, cfg)
        if self.dims.head_dim not in (64, 128) or self.dims.hidden > 4096:
            raise NotImplementedError(f"head_dim {self.dims.head_dim} / hidden {self.dims.hidden}: the MI355X engine serves head_dim 64 or 128 and "
                                      "hidden <= 4096 (Llama-2/3 up to 8B, Llama-3.2-1B, TinyLlama, SmolLM2, Qwen2.5-0.5B to 7B)")
        if self.dims.qk_norm and self.dims.head_dim != 128:            # (rk_engine_finalize refuses it too; no Qwen3 checkpoint has it)
            raise NotImplementedError(f"Qwen3 with head_dim {self.dims.head_dim}: the MI355X engine's q / k head norm is built for head_dim 128")
        if kv_dtype == "fp8" and self.dims.head_dim != 128:            # (rk_engine_finalize refuses it too)
            raise NotImplementedError(f"kv_dtype='fp8' with head_dim {self.dims.head_dim}: the MI355X engine's FP8 K / V cache is built for head_dim 128 "
                                      "(the 64-wide models' caches are small)")
        self.engine = RkLlamaEngine(self.dims, parse_device(device), max_tokens, max_seqs, **({"weight_fp8": True} if weight_dtype == "fp8" else {}),
                                    **({"kv_fp8": True} if kv_dtype == "fp8" else {}))
        tensors = iter_checkpoint_tensors(model_name_or_path)
        self.engine.load_state(merge_lora(tensors, adapter_dir) if adapter_dir else tensors)

    @classmethod
    def from_engine(cls, engine: RkLlamaEngine, dims=None) -> "LlamaRuntime":
        self = cls.__new__(cls)
        self.dims = dims if dims is not None else engine.dims
        self.config = self.dims.to_hf_config()
        self.model_type = self.config["model_type"]
        self.generation = read_generation_settings(None, self.config)
        self.max_tokens, self.max_seqs = int(engine.desc.max_tokens), int(engine.desc.max_seqs)
        self.engine = engine
        self.weight_dtype = "fp8" if getattr(engine, "weight_fp8", False) else "fp16"
        self.kv_dtype = "fp8" if getattr(engine, "kv_fp8", False) else "fp16"
        return self

    _chunks = T5Runtime._chunks
    _warned_sampling = False

    def generation_plan(self, prompt_lens) -> dict:
        """The arguments of `generate` for prompts of these lengths, from the checkpoint's generation settings in HF's order:
        max_new_tokens if set; else max_length (a limit on prompt + new tokens; a prompt that already reaches it raises what
        HF's generate raises); else the installed transformers' default.  do_sample: the engine decodes greedily and says so
        once."""
        return generation_plan(self, prompt_lens)

    sampling_on = False

    def set_sampling(self, temperature, top_k, top_p):
        """RkLlamaEngine.set_sampling; from then on `generate(..., seeds=...)` and a pool's `submit(..., seed=...)` sample
        (temperature 0: off again) and generation_plan has no deviation to warn of."""
        self.engine.set_sampling(temperature, top_k, top_p)
        self.sampling_on = float(temperature) > 0

    def generate(self, seqs, max_new, eos_ids, pad_id, max_total=0, seeds=None) -> np.ndarray:
        """[B, max_new] new tokens of every prompt (RkLlamaEngine.generate: prefill once, then one KV-cached row per token);
        chunked by capacity like T5Runtime.generate, the columns after the step at which every row of an engine call had
        finished hold -1.  A chunk leaves room for its continuations in the engine's token capacity.  seeds: one per prompt,
        the sampled form (a prompt's tokens depend on its own seed only, not on its chunk)."""
        parts = []
        done = 0
        for c in self._gen_chunks(seqs, max_new):
            if seeds is not None:
                toks, steps = self.engine.generate(c, max_new, eos_ids, pad_id, max_total, seeds=list(seeds[done:done + len(c)]))
                done += len(c)
            else:
                toks, steps = self.engine.generate(c, max_new, eos_ids, pad_id, max_total)
            toks = toks.copy()
            toks[:, steps:] = -1
            parts.append(toks)
        return np.concatenate(parts, axis=0)

    def _gen_chunks(self, seqs, max_new):
        for s in seqs:
            if len(s) + max_new > self.max_tokens:
                raise ValueError(f"a prompt of {len(s)} tokens + {max_new} new ones exceeds the engine capacity {self.max_tokens}")
        return self._chunks(seqs)

    def open_pool(self, max_new_cap, eos_ids, pad_id, n_slots=None, draft_tokens=0) -> "DecodePool":
        """A pool of `n_slots` (default: max_seqs) decoding slots over one engine session: requests are queued with `submit`,
        `wait` returns completed ones while the rest keep decoding, a finished row's slot goes to the next request.  A request's
        tokens are what `generate` gives for it alone.  A context manager; the engine's other calls are refused until it is
        closed.  draft_tokens = Kd in 1..7: a drafting session (RkLlamaEngine.session(draft=Kd): prompt-lookup drafts, the same
        tokens in fewer steps); every slot takes Kd + 1 of the step's max_seqs rows, so the default is max_seqs // (Kd + 1) slots."""
        draft = draft_tokens_kw(draft_tokens).get("draft_tokens", 0)
        n_slots = max(1, self.max_seqs // (draft + 1)) if n_slots is None else int(n_slots)
        if not 0 < n_slots * (draft + 1) <= self.max_seqs:
            raise ValueError(f"n_slots {n_slots}" + (f" x (draft_tokens {draft} + 1)" if draft else "") + f" outside 1..max_seqs {self.max_seqs}")
        eos_ids, pad_id = list(eos_ids), int(pad_id)
        kw = {"draft": draft} if draft else {}               # (without drafting: the call it always was)
        return DecodePool(lambda max_len: self.engine.session(n_slots, max_len, int(max_new_cap), eos_ids, pad_id, **kw),
                          n_slots, self.max_tokens, int(max_new_cap))

    def greedy1(self, seqs) -> np.ndarray:
        """next token (first arg-max of the last position's logits) of every prompt"""
        return np.concatenate([self.engine.greedy1(c) for c in self._chunks(seqs)], axis=0)

    def last_logits(self, seqs, out_ids) -> np.ndarray:
        return np.concatenate([self.engine.last_logits(c, out_ids) for c in self._chunks(seqs)], axis=0)

    # -- the three calls PointwiseLlmRanker makes (T5Runtime's names and shapes) ---------------------------------------------------
    def score(self, seqs, dec_prefix, out_ids) -> np.ndarray:
        """[n, len(out_ids)] logits of the position behind every prompt: T5Runtime.score's shape.  A decoder-only model has no
        decoder prefix - the prompt ends where the answer starts - so `dec_prefix` must be empty."""
        if len(dec_prefix):
            raise ValueError(f"a decoder-only model takes no decoder prefix (got {list(dec_prefix)}): the prompt carries it")
        if not len(seqs):
            return np.zeros((0, len(out_ids)), np.float32)
        return self.last_logits(seqs, out_ids)

    def qlm(self, seqs, labels) -> np.ndarray:
        """float32 [n]: log P(labels | prompt) of every prompt with the same labels (RkLlamaEngine.qlm on prompt + labels)."""
        return self.qlm_many(seqs, [labels] * len(seqs))

    def qlm_many(self, seqs, labels_per_seq) -> np.ndarray:
        """qlm scores of prompts with their OWN labels each (the passages of several queries): one engine call per capacity chunk
        of prompt + label tokens.  Element b is bit for bit what qlm gives seqs[b] with labels_per_seq[b]; an empty label list
        scores 0.0 without reaching the engine (the empty sum)."""
        if len(labels_per_seq) != len(seqs):
            raise ValueError(f"{len(seqs)} prompts but {len(labels_per_seq)} label sequences")
        out = np.zeros(len(seqs), np.float32)
        live = [b for b in range(len(seqs)) if len(labels_per_seq[b])]
        full = [list(seqs[b]) + list(labels_per_seq[b]) for b in live]
        done = 0
        for c in self._chunks(full):
            idx = live[done:done + len(c)]
            out[idx] = self.engine.qlm(c, [len(labels_per_seq[b]) for b in idx])
            done += len(c)
        return out

    def score_batches(self, batches, dec_prefix, out_ids) -> List[np.ndarray]:
        """T5Runtime.score_batches' contract: the batches merged up to the engine's capacity (a prompt's logits do not depend on
        what shares its call), the results cut back."""
        batches = list(batches)
        return self._cut(self.score([s for b in batches for s in b], dec_prefix, out_ids), batches)

    def qlm_batches(self, batches, labels) -> List[np.ndarray]:
        """T5Runtime.qlm_batches' contract, the same way."""
        batches = list(batches)
        return self._cut(self.qlm([s for b in batches for s in b], labels), batches)

    @staticmethod
    def _cut(rows, batches) -> List[np.ndarray]:
        out, pos = [], 0
        for b in batches:
            out.append(rows[pos:pos + len(b)])
            pos += len(b)
        return out


class DecodePool:
    """The scheduler between callers with many independent greedy requests and ONE decoding session (RkLlamaEngine.session, or a
    test double with its interface: n_slots, busy, admit, run, read, close).

    submit(key, ids, max_new) queues a request; the queue is FIFO.  wait() fills the free slots from the head of the queue - all
    of them in ONE admit, as far as the prefill's token capacity goes - runs the session until a slot finishes and returns
    [(key, new tokens)] of every request that completed (the EOS that ended a row included).  The session is opened at the first
    wait with max_len = the largest len + max_new queued, rounded up to LEN_STEP positions; a later request that needs more waits
    at the head of the queue until the running rows have drained, then the session is re-opened with the larger max_len (sizes
    never shrink, so the steady state re-opens and re-captures nothing)."""
    LEN_STEP = 512

    def __init__(self, open_session, n_slots: int, max_tokens: int, max_new_cap: int):
        self._open_session, self.n_slots, self.max_tokens, self.max_new_cap = open_session, int(n_slots), int(max_tokens), int(max_new_cap)
        self.session = None
        self.max_len = 0
        self._queue = []                    # [(key, ids, max_new, seed)] oldest first
        self._seeded = False                # the requests carry sampling seeds (submit)
        self._owner = {}                    # slot -> (key, prompt length)
        self.steps = self.admits = self.opens = self.tokens_out = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        """Ends the session whatever is still queued or decoding (the engine drains its stream): the engine is usable afterwards."""
        session, self.session = self.session, None
        self._queue.clear()
        self._owner.clear()
        if session is not None:
            session.close()

    def submit(self, key, ids, max_new: int, seed=None):
        """seed: the request's 64-bit sampling seed, for a pool over a session opened while sampling was on (every request of
        such a pool has one; a greedy pool's requests have none)."""
        ids, max_new = [int(t) for t in ids], int(max_new)
        if self._queue or self._owner:
            if (seed is None) != (not self._seeded):
                raise ValueError(f"request {key!r}: a pool's requests all carry a seed or none does")
        self._seeded = seed is not None
        if not ids or max_new <= 0:
            raise ValueError(f"request {key!r}: an empty prompt or max_new {max_new}")
        if max_new > self.max_new_cap:
            raise ValueError(f"request {key!r}: max_new {max_new} exceeds the pool's max_new_cap {self.max_new_cap}")
        if len(ids) + max_new > self.max_tokens:
            raise ValueError(f"request {key!r}: a prompt of {len(ids)} tokens + {max_new} new ones exceeds the engine capacity {self.max_tokens}")
        self._queue.append((key, ids, max_new, seed))

    @property
    def tokens_per_step(self) -> float:
        """new tokens of the completed requests per step issued so far (their first tokens, which the admits' prefills produce,
        included): about the number of busy slots for a plain session, more where drafts are accepted; 0.0 before the first step"""
        return self.tokens_out / self.steps if self.steps else 0.0

    def pending(self) -> int:
        """requests queued or decoding"""
        return len(self._queue) + len(self._owner)

    def _fill(self):
        """the head of the queue into the free slots: one admit"""
        if not self._queue:
            return
        need = max(len(ids) + max_new for _, ids, max_new, _ in self._queue)
        if self.session is None or (need > self.max_len and not self._owner):
            if self.session is not None:
                self.session.close()
                self.session = None
            step = self.LEN_STEP
            self.max_len = min(max(self.max_len, (need + step - 1) // step * step), self.max_tokens)
            self.session = self._open_session(self.max_len)
            self.opens += 1
        free = [s for s in range(self.n_slots) if s not in self.session.busy]
        take, tokens = [], 0
        for key, ids, max_new, seed in self._queue[:len(free)]:
            if len(ids) + max_new > self.max_len or tokens + len(ids) > self.max_tokens:
                break                       # (FIFO: nothing overtakes a request that waits for a larger session or the next prefill)
            take.append((key, ids, max_new, seed))
            tokens += len(ids)
        if not take:
            return
        slots = free[:len(take)]
        if self._seeded:
            self.session.admit([t[1] for t in take], slots, [t[2] for t in take], seeds=[t[3] for t in take])
        else:                               # (the greedy call shape, as every session double implements it)
            self.session.admit([t[1] for t in take], slots, [t[2] for t in take])
        self.admits += 1
        del self._queue[:len(take)]
        for slot, (key, ids, _, _) in zip(slots, take):
            self._owner[slot] = (key, len(ids))

    def wait(self):
        """Blocks until at least one request is complete -> [(key, tokens)]; [] when nothing is queued or decoding."""
        while self._queue or self._owner:
            self._fill()
            finished, steps = self.session.run()
            self.steps += steps
            done = []
            for slot in finished:
                key, _ = self._owner.pop(slot)
                tokens = np.asarray(self.session.read(slot), dtype=np.int32)
                self.tokens_out += len(tokens)
                done.append((key, tokens))
            if done:
                return done
            if not self._owner:             # (submit's checks rule it out: an empty session always takes the head of the queue)
                raise RuntimeError("the head of the queue fits neither the session nor the prefill")
        return []


def generation_plan(runtime, prompt_lens) -> dict:
    """LlamaRuntime.generation_plan for any runtime with a `generation` dict (the engine's, or a test double's)."""
    import logging
    g = runtime.generation
    if g.get("do_sample") and not getattr(runtime, "sampling_on", False) and not getattr(runtime, "_warned_sampling", False):
        logging.getLogger("llmrankers").warning(
            "the checkpoint's generation_config.json asks for sampling (do_sample: true); the MI355X engine decodes greedily "
            "unless the ranker is given sample_seed (opt-in, DESIGN.md section 4)")
        runtime._warned_sampling = True
    longest = max(prompt_lens)
    new, total = g.get("max_new_tokens"), g.get("max_length")
    if new is None and total is None:
        new, total = default_generation_length()
    if new is not None:
        max_new, max_total = int(new), 0
    else:
        max_total = int(total)
        if longest >= max_total:
            raise hf_prompt_too_long_error()(
                f"Input length of input_ids is {longest}, but `max_length` is set to {max_total}. This can lead to unexpected "
                "behavior. You should consider increasing `max_length` or, better yet, setting `max_new_tokens`.")
        max_new = max_total - min(prompt_lens)
    return {"max_new": max_new, "max_total": max_total, "eos_ids": list(g["eos_token_ids"]), "pad_id": int(g["pad_token_id"])}


def load_runtime(model_name_or_path: str, device, cache_dir=None, weight_dtype="fp16", kv_dtype="fp16"):
    """T5Runtime or LlamaRuntime by the checkpoint's config.model_type (ref: setwise.py:40-71 dispatches the same way);
    anything else raises NotImplementedError like the reference.  weight_dtype: LlamaRuntime's; "fp8" on a T5 checkpoint raises
    NotImplementedError.  kv_dtype: likewise."""
    path = resolve_checkpoint(model_name_or_path, cache_dir)
    mt = read_config(path).get("model_type")
    if mt == "t5":
        refuse_t5_weight_dtype(weight_dtype)
        refuse_t5_kv_dtype(kv_dtype)
        return T5Runtime(path, device, cache_dir=cache_dir)
    if mt == "llama":                                                 # (a default call makes the call it always made)
        return LlamaRuntime(path, device, cache_dir=cache_dir, **weight_dtype_kw(weight_dtype), **kv_dtype_kw(kv_dtype))
    raise NotImplementedError(f"Model type {mt} is not supported yet by the MI355X engine")
