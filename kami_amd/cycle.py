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
by kh_replay_add_device and rank 0 trains with NN.train_replay (kh_train_replay) from the ring in place."""
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


def generation(nn, pool, replay: "ReplayBuffer | CompactReplay | DeviceReplay", *, play_evals: int, play_seconds: float = 60.0, sample: int | None = None,
               mlr: int = 5, epochs: int = 8, batchsize: int = 8, momentum: float = 0.0, nesterov: bool = False,
               weight_decay: float = 0.0, max_grad_norm: float = 0.0, dist=None, device: str | None = None, gate: dict | None = None):
    """Play, collect, train (rank 0), publish.  Returns a dict of what happened.  The collectives' tensors live where
    the group's backend needs them (kd.collective_device: device memory for RCCL, host memory for gloo).
    gate=None: the trained weights are installed unconditionally.  gate=dict(...): rank 0 trains a clone of `nn`, plays
    search.Match(nn, clone, **gate) and installs the clone's weights and generation on `nn` only if it is accepted
    (selfplay.cpp:259-287); the result gains accepted, gate_score, gate_games.
    momentum / nesterov / weight_decay / max_grad_norm: NN.train's optimizer options, passed to either training path."""
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
    for r, blob in enumerate(gather_compact(dist, payload, C.sizeof(S.Record), root=0, device=device, as_tensor=on_device)):
        if compact:
            if not on_device:
                added = replay.add_bytes(blob)
            elif blob.is_cuda and blob.device.index == replay.device:
                added = replay.add_tensor(blob)                              # stays in device memory under RCCL
            else:
                added = replay.add_bytes(blob.cpu().numpy().tobytes())
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
