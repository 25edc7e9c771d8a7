"""kb_sense_contacts restated in numpy from the definition in include/kilobots_hip.h: a pure function of the warm-start
store (ws_cnt, ws_key, ws_acc).  Plain loops over the packed list, python sorting, no code shared with the kernel."""
import numpy as np

from tests import objects_ref

KEY_WALL, KEY_OBJ = 0x10000, 0x20000
WALL_PUBLIC = (0, 2, 1, 3)      # store: xmin ymin xmax ymax -> public (kb_sense_objects): xmin xmax ymin ymax


bits = objects_ref.bits


def quant(acc, scale):
    """The fixed-point image of KB_REDUCE_SUM: NaN -> 0, otherwise rint(clamp(acc * scale, +-2^21)), one fp32 product."""
    t = np.float32(acc) * np.float32(scale)
    if np.isnan(t):
        return 0
    return int(np.rint(np.clip(t, np.float32(-2097152.0), np.float32(2097152.0))))


def fixed_sum(q, scale):
    """(float)(int32)(sum modulo 2^32) / scale: int -> float to nearest even, one fp32 division."""
    s = int(q) & 0xFFFFFFFF
    s = s - (1 << 32) if s >= (1 << 31) else s
    return np.float32(np.float32(s) / np.float32(scale))


def entries(ws_cnt, ws_key, ws_acc, cap):
    """[(owner, key, acc)] of one env: the entries the store holds, owners ascending, those behind the capacity left out."""
    out, pos0 = [], 0
    for a, c in enumerate(np.asarray(ws_cnt).astype(np.int64)):
        for s in range(int(c)):
            pos = pos0 + s
            if pos < cap:
                out.append((a, int(np.uint32(ws_key[pos])), np.float32(ws_acc[pos])))
        pos0 += int(c)
    return out


def classify(a, key, N, fixture_body):
    """(class, code, fixture) of an entry of owner a: class 'k' kilobot, 'w' wall, 'o' object fixture, None ignored."""
    if key < N:
        return ('k', key, 0) if key != a else (None, 0, 0)
    if KEY_WALL <= key < KEY_WALL + 4:
        return 'w', N + WALL_PUBLIC[key - KEY_WALL], 0
    if key >= KEY_OBJ and key - KEY_OBJ < len(fixture_body):
        f = key - KEY_OBJ
        return 'o', N + 4 + int(fixture_body[f]), f
    return None, 0, 0


def env_lists(ws_cnt, ws_key, ws_acc, cap, N, fixture_body):
    """Per kilobot of one env the full ordered list [(code, fixture, acc bits, class)], both sides of every kilobot pair."""
    lists = [[] for _ in range(N)]
    for a, key, acc in entries(ws_cnt, ws_key, ws_acc, cap):
        cls, code, f = classify(a, key, N, fixture_body)
        if cls is None:
            continue
        b = int(np.float32(acc).view(np.uint32))
        lists[a].append((code, f, b, cls))
        if cls == 'k':
            lists[key].append((a, 0, b, cls))
    for l in lists:
        l.sort(key=lambda t: (((t[0] * 8 + t[1]) << 32) | t[2]))
    return lists


def contacts_ref(ws_cnt, ws_key, ws_acc, cap, N, M, fixture_body, k, scale=65536.0):
    """(partner [E, N, k] int32, impulse [E, N, k] float32, touch [E, N, 4] float32, obj [E, M, 2] float32 or None);
    partner and impulse are None with k = 0.  fixture_body: the body of every fixture in the kb_config numbering
    (range(M) for a handle with num_fixtures == 0)."""
    ws_cnt, ws_key, ws_acc = np.asarray(ws_cnt), np.asarray(ws_key).view(np.uint32), np.asarray(ws_acc, dtype=np.float32)
    E = ws_cnt.shape[0]
    partner = np.full((E, N, k), -1, np.int32) if k else None
    impulse = np.zeros((E, N, k), np.uint32) if k else None
    touch = np.zeros((E, N, 4), np.float32)
    obj = np.zeros((E, M, 2), np.float32) if M else None
    for e in range(E):
        lists = env_lists(ws_cnt[e], ws_key[e], ws_acc[e], cap, N, fixture_body)
        oq = [[0, 0] for _ in range(M)]
        for a, l in enumerate(lists):
            for i, (code, f, b, cls) in enumerate(l[:k]):
                partner[e, a, i] = code
                impulse[e, a, i] = b
            qs = 0
            for code, f, b, cls in l:
                q = quant(np.uint32(b).view(np.float32), scale)
                qs += q
                if cls == 'o':
                    oq[code - N - 4][0] += 1
                    oq[code - N - 4][1] += q
            touch[e, a] = (sum(t[3] == 'k' for t in l), sum(t[3] == 'w' for t in l), sum(t[3] == 'o' for t in l), fixed_sum(qs, scale))
        for m in range(M):
            obj[e, m] = (oq[m][0], fixed_sum(oq[m][1], scale))
    return partner, None if impulse is None else impulse.view(np.float32), touch, obj
