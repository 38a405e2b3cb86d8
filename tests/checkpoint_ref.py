"""A numpy reader and writer of the training-state checkpoint container (DESIGN.md §4 "Training-state checkpoints";
ppo.c_amd/host/checkpoint.c is the library's).  Written from the format's description, not from the C code: the tests
hold one against the other.

The image is little-endian: the magic PPOSTATE, u32 version (1), u32 flags, u32 section count; then per section
{u32 tag, u32 reserved = 0, u64 payload bytes, u64 FNV-1a-64 of the payload} and the payload, zero-padded to 8 bytes.
"""
import struct

import numpy as np

MAGIC = b"PPOSTATE"
VERSION = 1
HEADER, SECTION = 20, 24
LEGACY, SETTINGS, NORMALISERS, SHUFFLE, ROLLOUT, BUFFER = 1, 2, 3, 4, 5, 6
NAMES = {LEGACY: "legacy", SETTINGS: "settings", NORMALISERS: "normalisers", SHUFFLE: "shuffle", ROLLOUT: "rollout",
         BUFFER: "buffer"}
F_BUFFER, F_ROLLOUT = 1, 2          # header flags: a Buffer / a Rollout section follows
ENV_EXTERNAL = 3
MD_MAX_D = 256
F32, F64, U8, U32, I32 = np.float32, np.float64, np.uint8, np.uint32, np.int32


class CheckpointError(ValueError):
    pass


def fnv1a64(data):
    h = 0xcbf29ce484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def pad8(n):
    return (n + 7) & ~7


# ------------------------------------------------------------------------------------------- the container
def section_bytes(tag, payload, length=None, checksum=None, reserved=0):
    """one section; `length` / `checksum` / `reserved` override what the payload implies (for the decline tests)"""
    payload = bytes(payload)
    n = len(payload) if length is None else length
    c = fnv1a64(payload) if checksum is None else checksum
    return struct.pack("<IIQQ", tag, reserved, n, c) + payload + b"\0" * (pad8(len(payload)) - len(payload))


def write_image(sections, flags=None, version=VERSION, count=None, magic=MAGIC):
    """sections: [(tag, payload bytes)] in file order.  flags default to what the sections imply."""
    if flags is None:
        tags = [t for t, _ in sections]
        flags = (F_BUFFER if BUFFER in tags else 0) | (F_ROLLOUT if ROLLOUT in tags else 0)
    out = magic + struct.pack("<III", version, flags, len(sections) if count is None else count)
    return out + b"".join(section_bytes(t, p) for t, p in sections)


def read_image(data):
    """→ (version, flags, [(tag, payload bytes)]) with every section, unknown tags included; the container's own
    rules are checked: magic, version, count, reserved words, bounds, checksums, zero padding, no trailing bytes"""
    data = bytes(data)
    if len(data) < HEADER:
        raise CheckpointError("shorter than the header")
    if data[:8] != MAGIC:
        raise CheckpointError("bad magic")
    version, flags, count = struct.unpack_from("<III", data, 8)
    if version != VERSION:
        raise CheckpointError("unsupported version")
    if flags & ~(F_BUFFER | F_ROLLOUT):
        raise CheckpointError("unknown header flags")
    if count > (len(data) - HEADER) // SECTION:
        raise CheckpointError("more sections than the file could hold")
    pos, sections = HEADER, []
    for _ in range(count):
        if len(data) - pos < SECTION:
            raise CheckpointError("truncated inside a section header")
        tag, reserved, n, c = struct.unpack_from("<IIQQ", data, pos)
        if reserved:
            raise CheckpointError(f"section {tag}: reserved word not zero")
        pos += SECTION
        if pad8(n) > len(data) - pos:
            raise CheckpointError(f"section {tag}: payload runs past the end of the file")
        payload = data[pos:pos + n]
        if fnv1a64(payload) != c:
            raise CheckpointError(f"section {tag}: checksum mismatch")
        if any(data[pos + n:pos + pad8(n)]):
            raise CheckpointError(f"section {tag}: padding not zero")
        sections.append((tag, payload))
        pos += pad8(n)
    if pos != len(data):
        raise CheckpointError("bytes beyond the last section")
    return version, flags, sections


# ------------------------------------------------------------------------------------------- the sections
def legacy_header(p):
    if len(p) < 32:
        raise CheckpointError("legacy: shorter than its header")
    lam, eps, ent, lr_p, lr_v, S, A, cap = struct.unpack_from("<5f3i", p, 0)
    return dict(lam=lam, epsilon=eps, ent_coeff=ent, lr_policy=lr_p, lr_V=lr_v, S=S, A=A, cap=cap)


SETTING_KEYS = ("max_grad_norm", "target_kl", "value_clip", "obs_clip", "obs_frozen", "rew_clip", "rew_frozen",
                "ep_gamma", "action_dist", "nvec", "mask_on", "dtype_V", "dtype_mu")


def pack_settings(s):
    nvec = list(s["nvec"])
    return (struct.pack("<4fIfIfII", s["max_grad_norm"], s["target_kl"], s["value_clip"], s["obs_clip"],
                        s["obs_frozen"], s["rew_clip"], s["rew_frozen"], s["ep_gamma"], s["action_dist"], len(nvec))
            + np.asarray(nvec, "<i4").tobytes() + struct.pack("<III", s["mask_on"], s["dtype_V"], s["dtype_mu"]))


def parse_settings(p):
    if len(p) < 52:
        raise CheckpointError("settings: too short")
    v = struct.unpack_from("<4fIfIfII", p, 0)
    D = v[9]
    if v[8] > 2 or D > MD_MAX_D or (D != 0) != (v[8] == 2) or len(p) != 52 + 4 * D:
        raise CheckpointError("settings: distribution, component count and length disagree")
    nvec = np.frombuffer(p, "<i4", D, 40).tolist()
    mask_on, dt_v, dt_mu = struct.unpack_from("<III", p, 40 + 4 * D)
    if max(v[4], v[6], mask_on, dt_v, dt_mu) > 1 or (mask_on and v[8] == 0):
        raise CheckpointError("settings: a flag or dtype out of range")
    return dict(zip(SETTING_KEYS, v[:9] + (nvec, mask_on, dt_v, dt_mu)))


def pack_normalisers(obs, rew):
    """obs: the 1 + 2S doubles {n, mean[S], M2[S]} or None (never allocated); rew: {n, mean, M2}"""
    return (b"" if obs is None else np.asarray(obs, "<f8").tobytes()) + np.asarray(rew, "<f8").tobytes()


def parse_normalisers(p, S):
    if len(p) == 24:
        return None, np.frombuffer(p, "<f8", 3)
    if len(p) != 24 + 8 * (1 + 2 * S):
        raise CheckpointError("normalisers: the observation triple is not 1 + 2S doubles")
    return np.frombuffer(p, "<f8", 1 + 2 * S), np.frombuffer(p, "<f8", 3, 8 * (1 + 2 * S))


def pack_shuffle(key, seed, seeded):
    return struct.pack("<QQI", key, seed, seeded)


def parse_shuffle(p):
    if len(p) != 20:
        raise CheckpointError("shuffle: bad length")
    key, seed, seeded = struct.unpack("<QQI", p)
    if seeded > 1:
        raise CheckpointError("shuffle: bad flag")
    return dict(key=key, seed=seed, seeded=seeded)


def env_state_floats(S):
    return max(S, 5)


def _pad(b):
    return b + b"\0" * (pad8(len(b)) - len(b))


def pack_rollout(r):
    E, S = r["E"], r["S"]
    out = struct.pack("<4IQII", E, r["T"], r["kind"], S, r["step"], r["laid"], r["rew_scanned"])
    if r["kind"] != ENV_EXTERNAL:
        out += _pad(np.asarray(r["env_state"], "<f4").reshape(E, env_state_floats(S)).tobytes())
    out += _pad(np.asarray(r["cont"], U8).reshape(E).tobytes())
    out += np.asarray(r["carry_in"], "<f8").reshape(E).tobytes() + np.asarray(r["carry_out"], "<f8").reshape(E).tobytes()
    out += struct.pack("<II", r["ep_fresh"], r["ext_done"])
    out += np.asarray(r["ep_state"], "<f8").reshape(E, 4).tobytes() + np.asarray(r["ep_agg"], "<f8").reshape(16).tobytes()
    out += struct.pack("<Q", r["ext_key"])
    if r["ext_done"]:
        out += np.asarray(r["ext_obs"], "<f4").reshape(E, S).tobytes()
    return out


def parse_rollout(p, S, cap):
    if len(p) < 32:
        raise CheckpointError("rollout: too short")
    E, T, kind, roS, step, laid, scanned = struct.unpack_from("<4IQII", p, 0)
    if not (1 <= E < 2 ** 31 and 1 <= T < 2 ** 31 and E * T <= cap and kind <= ENV_EXTERNAL and roS == S
            and laid <= 1 and scanned <= 1):
        raise CheckpointError("rollout: shapes contradict the legacy header")
    env = 0 if kind == ENV_EXTERNAL else 4 * E * env_state_floats(S)
    base = 32 + pad8(env) + pad8(E) + 16 * E + 8 + 32 * E + 128 + 8
    if len(p) < base:
        raise CheckpointError("rollout: length contradicts its shapes")
    r = dict(E=E, T=T, kind=kind, S=S, step=step, laid=laid, rew_scanned=scanned)
    off = 32
    if env:
        r["env_state"] = np.frombuffer(p, "<f4", E * env_state_floats(S), off).reshape(E, -1)
        off += pad8(env)
    r["cont"] = np.frombuffer(p, U8, E, off)
    off += pad8(E)
    r["carry_in"] = np.frombuffer(p, "<f8", E, off)
    r["carry_out"] = np.frombuffer(p, "<f8", E, off + 8 * E)
    off += 16 * E
    r["ep_fresh"], r["ext_done"] = struct.unpack_from("<II", p, off)
    off += 8
    if r["ep_fresh"] > 1 or r["ext_done"] > 1 or (r["ext_done"] and kind != ENV_EXTERNAL):
        raise CheckpointError("rollout: a flag out of range")
    if len(p) != base + (4 * E * S if r["ext_done"] else 0):
        raise CheckpointError("rollout: length contradicts its shapes")
    r["ep_state"] = np.frombuffer(p, "<f8", 4 * E, off).reshape(E, 4)
    off += 32 * E
    r["ep_agg"] = np.frombuffer(p, "<f8", 16, off)
    off += 128
    r["ext_key"], = struct.unpack_from("<Q", p, off)
    off += 8
    if r["ext_done"]:
        r["ext_obs"] = np.frombuffer(p, "<f4", E * S, off).reshape(E, S)
    return r


def pack_buffer(b):
    n = b["limit"]
    out = struct.pack("<4I", b["idx"], b["full"], n, b["W"])
    for k, dt in (("state", "<f4"), ("action", "<f4"), ("logprob", "<f4"), ("reward", "<f4"), ("next_state", "<f4"),
                  ("terminated", U8), ("truncated", U8)):
        out += np.asarray(b[k], dt).reshape(n, -1).tobytes()
    out += b"\0" * (-len(out) % 4)
    if b["W"]:
        out += np.asarray(b["mask"], "<u4").reshape(n, b["W"]).tobytes()
    return out


def parse_buffer(p, S, A, cap, mask_on):
    if len(p) < 16:
        raise CheckpointError("buffer: too short")
    idx, full, n, W = struct.unpack_from("<4I", p, 0)
    if full > 1 or idx > cap or n != (cap if full else idx):
        raise CheckpointError("buffer: idx / full / limit contradict the capacity")
    if W != ((A + 31) // 32 if mask_on else 0):
        raise CheckpointError("buffer: mask words contradict the settings")
    if len(p) != 16 + 4 * n * (2 * S + A + 2) + ((2 * n + 3) & ~3) + 4 * n * W:
        raise CheckpointError("buffer: length contradicts its shapes")
    b, off = dict(idx=idx, full=full, limit=n, W=W), 16
    for k, dt, w in (("state", "<f4", S), ("action", "<f4", A), ("logprob", "<f4", 1), ("reward", "<f4", 1),
                     ("next_state", "<f4", S), ("terminated", U8, 1), ("truncated", U8, 1)):
        b[k] = np.frombuffer(p, dt, n * w, off).reshape(n, w)
        off += n * w * np.dtype(dt).itemsize
    off += -off % 4
    if W:
        b["mask"] = np.frombuffer(p, "<u4", n * W, off).reshape(n, W)
    return b


def parse(data):
    """the whole image → {"version", "flags", "legacy" (the raw stream), "header" (its shapes), "settings",
    "normalisers" (obs | None, rew), "shuffle", "rollout" | None, "buffer" | None, "unknown": [(tag, payload)]}, with
    the checks a reader owes: the required sections once each, the header's flags against the optional sections, every
    section's length against the shapes in the legacy header"""
    version, flags, sections = read_image(data)
    by_tag, unknown = {}, []
    for tag, payload in sections:
        if tag not in NAMES:
            unknown.append((tag, payload))          # skipped: a later version's section
        elif tag in by_tag:
            raise CheckpointError(f"section {tag} appears twice")
        else:
            by_tag[tag] = payload
    for tag in (LEGACY, SETTINGS, NORMALISERS, SHUFFLE):
        if tag not in by_tag:
            raise CheckpointError(f"section {tag}: a required section is missing")
    if bool(flags & F_BUFFER) != (BUFFER in by_tag) or bool(flags & F_ROLLOUT) != (ROLLOUT in by_tag):
        raise CheckpointError("the header's flags and the optional sections disagree")
    h = legacy_header(by_tag[LEGACY])
    if not (0 < h["S"] <= 1 << 24 and 0 < h["A"] <= 1 << 24 and h["cap"] >= 0):
        raise CheckpointError("legacy: bad shapes")
    out = dict(version=version, flags=flags, legacy=by_tag[LEGACY], header=h, unknown=unknown,
               settings=parse_settings(by_tag[SETTINGS]), normalisers=parse_normalisers(by_tag[NORMALISERS], h["S"]),
               shuffle=parse_shuffle(by_tag[SHUFFLE]), rollout=None, buffer=None)
    if ROLLOUT in by_tag:
        out["rollout"] = parse_rollout(by_tag[ROLLOUT], h["S"], h["cap"])
        if out["rollout"]["laid"] and not flags & F_BUFFER:
            raise CheckpointError("rollout: rollout-laid without the buffer")
    if BUFFER in by_tag:
        out["buffer"] = parse_buffer(by_tag[BUFFER], h["S"], h["A"], h["cap"], out["settings"]["mask_on"])
    return out
