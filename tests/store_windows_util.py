"""Helpers of the store-window tests: a tiny CALVIN-layout dataset directory written with numpy (reference dataset/README.md:50-119: one
episode_%07d.npz per time step, ep_start_end_ids.npy with inclusive ends, <lang_folder>/auto_lang_ann.npy, validation/<lang_folder>/embeddings.npy)."""
import os

import numpy as np

TRAIN_EPISODES = [(0, 39), (40, 64)]                       # 40 and 25 frames, inclusive frame ids
VAL_EPISODES = [(0, 29)]                                   # 30 frames
TRAIN_SEGMENTS = [(3, 20), (42, 55), (22, 39)]             # annotated (start, end) frame ids, inclusive; each inside one episode
VAL_SEGMENTS = [(2, 14), (15, 29)]
TASKS = ["open_drawer", "push_block", "open_drawer"]
SENTENCES = {"open_drawer": "open the drawer", "push_block": "push the block"}
LANG_FOLDER = "lang_annotations"


def _unit(rng, *shape):
    e = rng.standard_normal(shape).astype(np.float32)
    return e / np.linalg.norm(e, axis=-1, keepdims=True)


def write_split(d, episodes, segments, tasks, rng, with_embeddings=False, small_frames=False):
    os.makedirs(os.path.join(d, LANG_FOLDER), exist_ok=True)
    hs, hg = (8, 4) if small_frames else (200, 84)
    for a, e in episodes:
        for fid in range(a, e + 1):
            act = rng.uniform(-1, 1, 7).astype(np.float32)
            act[6] = 1.0 if rng.random() < 0.5 else -1.0
            ro = (rng.standard_normal(15) * 0.3).astype(np.float32)
            np.savez(os.path.join(d, f"episode_{fid:07d}.npz"), rgb_static=rng.integers(0, 256, (hs, hs, 3), dtype=np.uint8),
                     rgb_gripper=rng.integers(0, 256, (hg, hg, 3), dtype=np.uint8), rel_actions=act, actions=act, robot_obs=ro,
                     scene_obs=np.zeros(24, np.float32))
    np.save(os.path.join(d, "ep_start_end_ids.npy"), np.asarray(episodes, np.int64))
    ann = {"language": {"ann": [SENTENCES[t] for t in tasks], "task": list(tasks), "emb": _unit(rng, len(segments), 1, 384)},
           "info": {"indx": [tuple(s) for s in segments], "episodes": []}}
    np.save(os.path.join(d, LANG_FOLDER, "auto_lang_ann.npy"), ann, allow_pickle=True)
    if with_embeddings:
        emb = {t: {"emb": _unit(rng, 1, 1, 384), "ann": [s]} for t, s in SENTENCES.items()}
        np.save(os.path.join(d, LANG_FOLDER, "embeddings.npy"), emb, allow_pickle=True)


def write_dataset(root, seed=0, small_frames=False):
    """<root>/training: two episodes (40 + 25 frames), three annotated segments; <root>/validation: one episode of 30 frames, two segments."""
    rng = np.random.default_rng(seed)
    write_split(os.path.join(root, "training"), TRAIN_EPISODES, TRAIN_SEGMENTS, TASKS, rng, small_frames=small_frames)
    write_split(os.path.join(root, "validation"), VAL_EPISODES, VAL_SEGMENTS, TASKS[:2], rng, with_embeddings=True, small_frames=small_frames)
    return str(root)
