"""One generation of kami's outer loop on this stack: self-play -> replay records -> NN::train -> gating match
(optional: `gate`) -> new generation (kami/selfplay.cpp:58-304, the match of evaluate.cpp included).

    play      kami_amd.search.Pool          MCTS trees -> kh_encode_infer_legal           (rows f1, f2)
    collect   gather_compact + ReplayBuffer finished games' positions, merged over ranks as 664-byte records (row f3)
    train     NN.train (kh_train)           the reference's SGD loop on the device        (row f4)
    gate      kami_amd.search.Match         candidate against current, installed if accepted (selfplay.cpp:274)
    publish   dist.broadcast_weights        every rank's evaluator gets the new generation (row f3)

Multi-GPU: every rank plays its own shard of the trees with its own engine, rank 0 trains.

With a CompactReplay ring the records stay compact all the way: the gathered payloads go into the ring as bytes and rank 0
trains with NN.train_records (kh_train_records), which expands each batch on the device.  With a DeviceReplay ring
they also stay where the collective left them: under RCCL the gathered payloads are device tensors, go into the ring
by kh_replay_add_device and rank 0 trains with NN.train_replay (kh_train_replay) from the ring in place.

Hold-out (`holdout`, `holdout_pct`): the tail of every rank's gathered payload goes into a second DeviceReplay ring that
is never trained on, and rank 0 reports the served network's loss on it (NN.eval_replay, kh_eval_replay) before and
after training."""
from __future__ import annotations

import numpy as np

from . import _lib as L
from . import dist as kd
from .replay import CompactReplay, DeviceReplay, ReplayBuffer

OBSIZE, PSIZE = 8 * 8 * 30, 4672


def records_to_arrays(nn, records):
    """ks_record[] -> (planes [n,1920] fp32 via the device encoder, dense visit rows [n,4672], values [n])."""
    n = len(records)
    boards = np.frombuffer(b"".join(bytes(r.board) for r in records), dtype=L.BOARD_DTYPE) if n else np.zeros(0, L.BOARD_DTYPE)
    planes = nn.encode(boards).reshape(n, OBSIZE) if n else np.zeros((0, OBSIZE), np.float32)
    mcts = np.zeros((n, PSIZE), np.float32)
    vals = np.zeros(n, np.float32)
    for i, r in enumerate(records):
        mcts[i, list(r.actions[:r.nact])] = r.visits[:r.nact]
        vals[i] = r.value
    return planes, mcts, vals


def split_holdout(payload, record_bytes: int, pct: int):
    """One rank's payload of k whole records -> (train, held): the LAST k * pct // 100 records are held out, the rest
    train.  A contiguous tail keeps the positions of whole games together (records arrive game by game), apart from the
    one game the cut may fall into.  `payload`: bytes, or a 1-D uint8 torch tensor, which is sliced where it lies (a
    device tensor never visits the host).  ValueError for a length that is not a whole number of records or a pct
    outside [0, 50]."""
    if not 0 <= pct <= 50:
        raise ValueError(f"holdout_pct {pct} outside [0, 50]")
    size = len(payload) if isinstance(payload, (bytes, bytearray, memoryview)) else payload.numel()
    if record_bytes < 1 or size % record_bytes:
        raise ValueError(f"{size} bytes are not a whole number of {record_bytes}-byte records")
    k = size // record_bytes
    cut = (k - k * pct // 100) * record_bytes
    return payload[:cut], payload[cut:]


def _add_payload(ring, blob) -> int:
    """A rank's payload (bytes, or a uint8 tensor as gather_compact(as_tensor=True) returns it) into a compact ring."""
    if isinstance(blob, (bytes, bytearray, memoryview)):
        return ring.add_bytes(bytes(blob))
    if isinstance(ring, DeviceReplay) and blob.is_cuda and blob.device.index == ring.device:
        return ring.add_tensor(blob)                                         # stays in device memory under RCCL
    return ring.add_bytes(blob.cpu().numpy().tobytes())


def generation(nn, pool, replay: "ReplayBuffer | CompactReplay | DeviceReplay", *, play_evals: int, play_seconds: float = 60.0, sample: int | None = None,
               mlr: int = 5, epochs: int = 8, batchsize: int = 8, momentum: float = 0.0, nesterov: bool = False,
               weight_decay: float = 0.0, max_grad_norm: float = 0.0, dist=None, device: str | None = None, gate: dict | None = None,
               holdout: "DeviceReplay | None" = None, holdout_pct: int = 0):
    """Play, collect, train (rank 0), publish.  Returns a dict of what happened.  The collectives' tensors live where
    the group's backend needs them (kd.collective_device: device memory for RCCL, host memory for gloo).
    gate=None: the trained weights are installed unconditionally.  gate=dict(...): rank 0 trains a clone of `nn`, plays
    search.Match(nn, clone, **gate) and installs the clone's weights and generation on `nn` only if it is accepted
    (selfplay.cpp:259-287); the result gains accepted, gate_score, gate_games.
    momentum / nesterov / weight_decay / max_grad_norm: NN.train's optimizer options, passed to either training path.
    holdout=DeviceReplay, holdout_pct in [1, 50] (both or neither; ValueError otherwise, before anything is played): of
    every rank's gathered payload split_holdout() puts the tail into `holdout`, which nothing trains on, and the rest into
    `replay`; the result gains held_out (records put aside by this call) and, once `holdout` holds records,
    holdout_before / holdout: NN.eval_replay of `nn` before training and of the trained network (the clone under a
    gate) after it and before the match, as dicts of EvalResult's fields."""
    hold = holdout is not None or holdout_pct != 0
    if hold:
        if not isinstance(holdout, DeviceReplay):
            raise ValueError("holdout must be a DeviceReplay ring (kh_eval_replay reads a device ring)")
        if isinstance(holdout_pct, bool) or not isinstance(holdout_pct, int) or not 1 <= holdout_pct <= 50:
            raise ValueError(f"holdout_pct {holdout_pct!r} outside [1, 50]")
    device = device or kd.collective_device(dist)
    import ctypes as C
    from . import search as S
    from .replay import gather_compact
    st = pool.run(min_evals=play_evals, max_seconds=play_seconds)
    on_device = isinstance(replay, DeviceReplay)
    compact = on_device or isinstance(replay, CompactReplay)
    # merge over the ranks as COMPACT records (664 B each); into a dense ring the root expands them (device encoder)
    if compact:
        payload = pool.drain_bytes()
        mine = range(len(payload) // C.sizeof(S.Record))
    else:
        mine = pool.drain()
        payload = b"".join(bytes(r) for r in mine)
    merged = 0
    rank0 = dist is None or dist.get_rank() == 0
    held_out = 0
    for r, blob in enumerate(gather_compact(dist, payload, C.sizeof(S.Record), root=0, device=device, as_tensor=on_device)):
        if hold:
            blob, held = split_holdout(blob, C.sizeof(S.Record), holdout_pct)
            held_out += _add_payload(holdout, held)
        if compact:
            added = _add_payload(replay, blob)
            if dist is not None and r != dist.get_rank():
                merged += added
            continue
        recs = (S.Record * (len(blob) // C.sizeof(S.Record))).from_buffer_copy(blob)
        planes, mcts, vals = records_to_arrays(nn, recs)
        for i in range(len(vals)):
            replay.add(planes[i], mcts[i], float(vals[i]))                  # selfplay.cpp:176-184
        if dist is not None and r != dist.get_rank():
            merged += len(vals)
    if not rank0:
        merged = 0
    vals = mine
    rank = dist.get_rank() if dist is not None else 0
    out = {"evals": st.evals, "games_finished": st.games_finished, "records": len(vals), "merged": merged,
           "generation_before": nn.get_generation()}
    if hold:
        out["held_out"] = held_out
    held_have = min(holdout.count(), holdout.size()) if hold and rank == 0 else 0
    if held_have:
        out["holdout_before"] = nn.eval_replay(holdout).as_dict()
    have = min(replay.count(), replay.size())
    optim = dict(momentum=momentum, nesterov=nesterov, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    trainee = nn.clone() if gate is not None and rank == 0 and have >= batchsize else nn      # selfplay.cpp:259
    if rank == 0 and have >= batchsize and compact:
        n = sample or (have // batchsize) * batchsize
        if on_device:
            first, last = trainee.train_replay(replay, n, mlr=mlr, epochs=epochs, batchsize=batchsize, **optim)
        else:
            first, last = trainee.train_records(replay.select(n), mlr=mlr, epochs=epochs, batchsize=batchsize, **optim)
        out.update(first_loss=first, last_loss=last, trained_on=n)
    elif rank == 0 and have >= batchsize:
        n = sample or (have // batchsize) * batchsize
        src = replay._rng.integers(0, have, n)                               # replaybuffer.h:61-84, over the written slots
        first, last = trainee.train(replay.input_buffer[src].reshape(n, 8, 8, 30), replay.mcts_buffer[src], replay.result_buffer[src],
                               mlr=mlr, epochs=epochs, batchsize=batchsize, **optim)
        out.update(first_loss=first, last_loss=last, trained_on=n)
    if held_have:
        out["holdout"] = trainee.eval_replay(holdout).as_dict() if "trained_on" in out else dict(out["holdout_before"])
    if gate is not None:
        out.update(accepted=False, gate_score=0.0, gate_games=0)             # (nothing trained, or not the training rank)
    if trainee is not nn:
        res = S.Match(nn, trainee, **gate).run()                             # selfplay.cpp:274
        out.update(accepted=bool(res.accepted), gate_score=res.score, gate_games=res.games_counted)
        if res.accepted:
            nn.load_weights(trainee.get_weights(), trainee.get_generation())
        trainee.close()
    if dist is not None:
        blob, gen = kd.broadcast_weights(dist, nn.get_weights() if rank == 0 else None, nn.get_generation() if rank == 0 else 0,
                                         src=0, device=device, as_tensor=True)      # stays in device memory under RCCL
        if rank != 0:
            if blob.is_cuda and blob.device.index != nn.cfg.device:     # an engine on another GPU than the collective's tensor
                blob = blob.cpu()
            nn.load_weights(blob, gen)
    out["generation_after"] = nn.get_generation()
    return out
