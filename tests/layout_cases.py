"""The layout and weight-pack kernels of csrc/layout.hip against independent references at their tile, job-count, route and view
edges: case tables, references, gates and the runners that the host test (tests/test_layout_cases_host.py, CPU model of the ABI) and
the GPU test (tests/test_gpu_layout_kernels.py, libvinet_hip.so) share.  Nothing here shares code with tests/abi_emulator.py.

Almost everything in this family is a permutation, one rounding or one fp32 add, so bit equality comes first.  u = 2^-24.

  pack, F32 / BF16     bit-equal to the array built by indexing from the formats written in layout.hip: forward out[t][n][c],
                       transposed out[t][c][n], stem out[kh][n][kw*4 + c], padding columns +0, for `ld` jobs only the columns
                       [col, col + N) of each row written.  bf16 is tensor.to(torch.bfloat16) (round to nearest even).
  pack, F32S           hi = bf16(v), lo = bf16(v - hi) bit for bit (v - hi is exact in fp32: one right answer).  Positions come from
                       F32S_POS, written from the sentence of the format comment: K positions 8q .. 8q+7 of a 32-wide chunk hold
                       channels {4q .. 4q+3, 16+4q .. 16+4q+3}; hi at the position, lo 32 further on, 64 bf16 per chunk.  Inputs are
                       finite normals.
  every pack output    lies in ONE arena filled with the sentinel, 64 elements of it between two jobs and behind the last: the whole
                       arena is compared in its bits, so a write outside a job's own elements fails like a wrong value.
  unpack               grad bit-equal to torch's fp32 g + v (or v): one add.  With the clear flag every packed element of rows
                       [0, N) of every slice is +0 afterwards, padding columns included, and they arrive non-zero; without it the
                       workspace keeps its bits.  Both arenas carry the sentinel between jobs.
  import, import_pad   bit-equal: a copy and one rounding, +0 in the pad ring and in the channels [C, dst.C).
  export, copy_affine  two data sets per case.  EXACT: x integers in [-3, 3], scale in +-{0.5, 1, 2}, shift integers in [-4, 4], the
                       old destination integers in [-8, 8]: every result is a multiple of 0.5 of magnitude <= 18, exact in bf16, and no
                       negative zero can arise (both asserted on the reference); multiply-then-add and fmaf agree, so the gate is bit
                       equality on either side.  RANDOM: |got - ref| <= b = 2u (|x * scale| + |shift| + |old|), one rounding for the
                       fma and one for the add, the float64 reference starting from the stored inputs; a bf16 destination adds half a
                       bf16 ulp at |ref| + b (bn_cases.bf16_half_ulp).  (The CPU model fuses the affine of these entry points like the
                       kernels' fmaf: multiply, round, add takes three roundings, worst case 3u |x * scale| + 2u |shift| + u |old|,
                       and missed this gate on a random export case.)  ReLU is gated on the float64
                       sign of x * scale + shift (exact product, a rounded sum keeps its sign), as in bn_cases.
  split_bf16           hi == bf16(v) and lo == bf16(v - hi) bit for bit on exact data and on affine-free random data.  Random data
                       with the affine: hi + lo within b + 2^-16 (|v| + b) of the float64 v (|v - hi| <= 2^-8 |v|, its rounding to
                       bf16 another 2^-8 of that).
  every written view   sits in a buffer with the sentinel around it and a tail behind it (bn_cases.put_tailed); every read-only buffer
                       is compared with its initial bits afterwards.

The route of vinet_copy_affine (copy_route) and the tile shapes of the tiled pack (pt_shape, prefix_per) are mirrored here in Python
because no call names its kernel; the host test asserts that the tables reach what they claim through these mirrors.

NOT COVERED: the doubling of copy_affine8's voxels per block past 16 384 blocks (about 1 GB of tensors); C > 2048, which takes two
group passes and is in no net; element-wise launches at or past 2^31 items; vinet_debug_spin."""
import functools

import torch

from tests.bn_cases import NAN, SENTINEL, Vec, _gen, _pick, bf16_half_ulp, oct_ok, put_tailed, quad_ok, untailed, view_geo
from tests.tail_cases import BF16, DTN, F32, TDT, U32, Side, Slab, gate_bound      # noqa: F401 (Side: for the test modules)
from vinet_amd import _lib as L

F32S = L.F32S
PDTS = (F32, BF16, F32S)
PDTN = {F32: "f32", BF16: "bf16", F32S: "f32s"}
DTS = (F32, BF16)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = _bits(got), _bits(want)
    bad = a != b
    assert not bool(bad.any()), "%s: %d of %d elements differ in their bits, first at %r: %r against %r" % (
        what, int(bad.sum()), a.numel(), tuple(int(i) for i in bad.nonzero()[0]), float(got[bad][0]), float(want[bad][0]))
    return a.numel()


def dims_of(n):
    """(B, T, H, W) with B * T * H * W == n: two batch items and more than one frame wherever n allows"""
    B = 2 if n % 2 == 0 else 1
    m = n // B
    T = next((f for f in (2, 3, 5, 7) if m % f == 0), 1)
    m //= T
    H = max(d for d in range(1, int(m ** 0.5) + 1) if m % d == 0)
    assert B * T * H * (m // H) == n
    return B, T, H, m // H


# =====================================================================================================================
# weight packing: vinet_pack_weights, vinet_pack_weights_multi; vinet_unpack_wgrad, vinet_unpack_wgrad_multi
# =====================================================================================================================
PT_MAXJOBS, PT_LDS_FLOATS, PT_GRID = 1024, 8448, 2048
TAPS = (1, 27, 32, 33, 64, 65, 128, 129, 256, 257)
CLASS_TOP = (32, 64, 128, 256)          # the largest tap count of each tile class
JOB_COUNTS = (1, 255, 256, 257, 1024, 1025)

# K position of channel c of a 32-wide chunk in the split format: positions 8q .. 8q+7 hold channels {4q .. 4q+3, 16+4q .. 16+4q+3}
F32S_POS = [None] * 32
for _q in range(4):
    for _i, _c in enumerate(list(range(4 * _q, 4 * _q + 4)) + list(range(16 + 4 * _q, 16 + 4 * _q + 4))):
        F32S_POS[_c] = 8 * _q + _i
assert sorted(F32S_POS) == list(range(32))


def pt_pairs(ntaps):
    return 256 if ntaps <= 32 else 128 if ntaps <= 64 else 64 if ntaps <= 128 else 32


def pt_shape(N, Cin, ntaps, transpose=False, stem=False, has_ld=False):
    """csrc/layout.hip pt_shape: dict(TRn, TCc, tilesR, tilesC, rs, units); TRn == 0: 256 packed elements per unit"""
    rup32 = lambda v: (v + 31) // 32 * 32
    if stem:
        return dict(TRn=0, TCc=0, tilesR=0, tilesC=0, rs=0, units=(7 * N * 32 + 255) // 256)
    if ntaps > 256:
        return dict(TRn=0, TCc=0, tilesR=0, tilesC=0, rs=0, units=(ntaps * (Cin if transpose else N) * rup32(N if transpose else Cin) + 255) // 256)
    pairs = pt_pairs(ntaps)
    TCc, TRn = (8, pairs // 8) if transpose else (32, pairs // 32)
    Kp = rup32(N if transpose else Cin)
    extC = Cin if transpose else Kp
    extN = (N if has_ld else Kp) if transpose else N
    tilesC, tilesR = -(-extC // TCc), -(-extN // TRn)
    return dict(TRn=TRn, TCc=TCc, tilesR=tilesR, tilesC=tilesC, rs=TCc * ntaps + 1, units=tilesC * tilesR)


def prefix_per(njobs):
    """jobs per thread of pt_build_prefix"""
    return (njobs + 255) // 256


class PJob:
    """one row of a pack table.  dest: jobs of equal `dest` share one side-by-side destination (ld != 0)"""

    def __init__(self, N, Cin, ntaps, tr=0, stem=0, ld=0, col=0, dest=None):
        self.N, self.Cin, self.ntaps, self.tr, self.stem, self.ld, self.col, self.dest = N, Cin, ntaps, tr, stem, ld, col, dest
        self.rows = N if (stem or not tr) else Cin
        self.Kp = 32 if stem else ((N if tr else Cin) + 31) // 32 * 32
        self.nsl = 7 if stem else ntaps
        self.numel = self.nsl * self.rows * self.Kp                     # the job's share of `total` (the element-wise kernels' walk)
        self.dest_numel = self.nsl * self.rows * (ld or self.Kp)
        self.shape = pt_shape(N, Cin, ntaps, bool(tr), bool(stem), ld != 0)

    def unpack_ok(self):
        return not self.tr and not self.ld

    def __repr__(self):
        return "%dx%dx%d%s%s%s" % (self.N, self.Cin, self.ntaps, "T" if self.tr else "", "S" if self.stem else "", "@%d.%d" % (self.ld, self.col) if self.ld else "")


class PCase:
    def __init__(self, tag, jobs, single=True):
        self.tag, self.jobs, self.single = tag, jobs, single
        self.units = sum(j.shape["units"] for j in jobs)

    def __repr__(self):
        return self.tag


def shape_jobs(nt):
    """the jobs of one tap count: tile tails on both sides in both forms; at the largest tap count of a class also 1 x 1 and a job
    of whole tiles"""
    cls = pt_pairs(min(nt, 256))
    trf = cls // 32
    jobs = [PJob(n, c, nt) for n in (trf - 1, trf + 1) if n > 0 for c in (31, 33)]
    jobs += [PJob(n, c, nt, tr=1) for n in (31, 33) for c in (7, 9)]
    if nt in CLASS_TOP:
        jobs += [PJob(1, 1, nt), PJob(1, 1, nt, tr=1), PJob(trf, 32, nt), PJob(cls // 8, 32, nt, tr=1)]
    return jobs


def misc_jobs():
    """the stem twice; side-by-side destinations: ld = 96 at col 0 and 32, two taps at ld = 64, and the columns engine.py's joint
    conv of Mixed_4c produces (members of 160, 112 and 24 outputs: col 0, 160, 272 of rows of 320 -- 272 is no multiple of 32)"""
    return [PJob(64, 3, 49, stem=1), PJob(1, 4, 49, stem=1),
            PJob(24, 40, 1, tr=1, ld=96, col=0, dest="a"), PJob(50, 40, 1, tr=1, ld=96, col=32, dest="a"),
            PJob(20, 5, 2, tr=1, ld=64, col=0, dest="b"), PJob(30, 5, 2, tr=1, ld=64, col=32, dest="b"),
            PJob(160, 9, 1, tr=1, ld=320, col=0, dest="c"), PJob(112, 9, 1, tr=1, ld=320, col=160, dest="c"), PJob(24, 9, 1, tr=1, ld=320, col=272, dest="c")]


COUNT_CYCLE = ((3, 5, 1, 0, 0), (2, 3, 2, 1, 0), (1, 4, 49, 0, 1), (5, 2, 3, 0, 0), (4, 9, 1, 1, 0))        # (N, Cin, ntaps, tr, stem)


def count_jobs(njobs, unpack=False):
    return [PJob(N, Cin, nt, tr=0 if unpack else tr, stem=st) for N, Cin, nt, tr, st in (COUNT_CYCLE[j % 5] for j in range(njobs))]


PACK_CASES = ([PCase("taps%d" % nt, shape_jobs(nt)) for nt in TAPS] + [PCase("misc", misc_jobs())] +
              [PCase("njobs%d" % n, count_jobs(n), single=False) for n in JOB_COUNTS] +
              [PCase("units", [PJob(520, 1024, 1), PJob(33, 9, 27, tr=1), PJob(1, 4, 49, stem=1)], single=False)])
UNPACK_FLAGS = (0, 1, 2, 3)
UNPACK_CASES = ([(PCase("taps%d" % nt, [j for j in shape_jobs(nt) if j.unpack_ok()]), f) for nt in TAPS for f in UNPACK_FLAGS] +
                [(PCase("misc", [j for j in misc_jobs() if j.unpack_ok()]), f) for f in UNPACK_FLAGS] +
                [(PCase("njobs%d" % n, count_jobs(n, True), single=False), 3) for n in JOB_COUNTS] +
                [(PCase("njobs257", count_jobs(257, True), single=False), 0),
                 (PCase("units", [PJob(520, 1024, 1), PJob(33, 9, 27), PJob(1, 4, 49, stem=1)], single=False), 3)])
PACK_PATHS = ("single", "tiled", "elementwise")


def pack_kernel(path, dt, njobs, unpack=False):
    """the kernel a path launches"""
    if unpack:
        return {"single": "unpack_wgrad_kernel", "tiled": "unpack_wgrad_tiled_kernel" if njobs <= PT_MAXJOBS else "unpack_wgrad_multi_kernel",
                "elementwise": "unpack_wgrad_multi_kernel"}[path]
    name = {"single": "pack_weights_kernel", "tiled": "pack_weights_tiled_kernel" if njobs <= PT_MAXJOBS else "pack_weights_multi_kernel",
            "elementwise": "pack_weights_multi_kernel"}[path]
    return "%s<%s>" % (name, PDTN[dt])


def job_weight(case, j):
    job = case.jobs[j]
    return torch.randn((job.N, job.Cin, job.ntaps), generator=_gen("pack_w", case.tag, j))


def logical_pack(job, w, lg, mask):
    """the job's elements in the logical fp32 destination lg [slices, rows, row length] (mask: what the job writes)"""
    if job.stem:                                        # out[kh][n][kw*4 + c] = w[n][c][kh*7 + kw]
        lg[...] = 0.0
        for kh in range(7):
            for kw in range(7):
                lg[kh, :, kw * 4:kw * 4 + job.Cin] = w[:, :, kh * 7 + kw]
        mask[...] = True
    elif not job.tr:                                    # out[t][n][c]
        lg[...] = 0.0
        lg[:, :, :job.Cin] = w.permute(2, 0, 1)
        mask[...] = True
    elif not job.ld:                                    # out[t][c][n]
        lg[...] = 0.0
        lg[:, :, :job.N] = w.permute(2, 1, 0)
        mask[...] = True
    else:                                               # only the job's own columns
        lg[:, :, job.col:job.col + job.N] = w.permute(2, 1, 0)
        mask[:, :, job.col:job.col + job.N] = True


def encode_pack(lg, mask, dt, store):
    """write the masked elements of the flat logical array into `store` (the destination in its storage type)"""
    if dt == F32:
        store[mask] = lg[mask]
    elif dt == BF16:
        store[mask] = lg.bfloat16()[mask]
    else:
        n = lg.numel()
        assert n % 32 == 0 and store.numel() == 2 * n
        idx = torch.arange(n)
        pos = (idx // 32) * 64 + torch.tensor(F32S_POS)[idx % 32]
        hi = lg.bfloat16()
        lo = (lg - hi.float()).bfloat16()
        store[pos[mask]] = hi[mask]
        store[pos[mask] + 32] = lo[mask]


GAP = 64          # sentinel elements between two destinations (and the alignment of each)


def _pack_layout(case, dt):
    """-> ([(dest key, [job indices], offset, storage elements)], arena length) in storage elements"""
    k = 2 if dt == F32S else 1
    dests, seen = [], {}
    for j, job in enumerate(case.jobs):
        key = job.dest if job.ld else ("job", j)
        if key in seen:
            dests[seen[key]][1].append(j)
        else:
            seen[key] = len(dests)
            dests.append([key, [j], 0, job.dest_numel * k])
    off = GAP
    for d in dests:
        d[2] = off
        off = (off + d[3] + GAP + GAP - 1) // GAP * GAP
    return dests, off


def pack_expected(case, dt, skip_ld=False):
    """(the arena every path has to leave behind, bit for bit; [offset of each job's destination])"""
    sdt = torch.float32 if dt == F32 else torch.bfloat16
    dests, total = _pack_layout(case, dt)
    arena = torch.full((total,), SENTINEL).to(sdt)
    offs = [0] * len(case.jobs)
    for key, members, off, n in dests:
        j0 = case.jobs[members[0]]
        shape = (j0.nsl, j0.rows, j0.ld or j0.Kp)
        lg, mask = torch.zeros(shape), torch.zeros(shape, dtype=torch.bool)
        for j in members:
            offs[j] = off
            logical_pack(case.jobs[j], job_weight(case, j), lg, mask)
        if not (skip_ld and j0.ld):
            encode_pack(lg.reshape(-1), mask.reshape(-1), dt, arena[off:off + n])
    return arena, offs


def _weights_arena(case):
    ws = [job_weight(case, j).reshape(-1) for j in range(len(case.jobs))]
    offs, off = [], 0
    for w in ws:
        offs.append(off)
        off += (w.numel() + 3) // 4 * 4
    arena = torch.full((off + 4,), NAN)
    for w, o in zip(ws, offs):
        arena[o:o + w.numel()] = w
    return arena, offs


class pack_tiled:
    """`with pack_tiled(api, v)`: the option at v, back at 1 whatever happens"""

    def __init__(self, api, v):
        self.api, self.v = api, v

    def __enter__(self):
        assert self.api.vinet_set_option(b"pack_tiled", self.v) == 0

    def __exit__(self, *a):
        self.api.vinet_set_option(b"pack_tiled", 1)


def check_pack(side, case, dt, paths=PACK_PATHS):
    """every path of the case against the same arena"""
    es = 4 if dt == F32 else 2
    warena, woffs = _weights_arena(case)
    wdev = side.put(warena)
    ran = {}
    for path in paths:
        if path == "single" and not case.single:
            continue
        want, offs = pack_expected(case, dt, skip_ld=(path == "single"))
        out = side.put(torch.full((want.numel(),), SENTINEL).to(want.dtype))
        wp = lambda j: wdev.data_ptr() + 4 * woffs[j]
        op = lambda j: out.data_ptr() + es * offs[j]
        if path == "single":
            for j, job in enumerate(case.jobs):
                if not job.ld:
                    side.call("vinet_pack_weights", wp(j), job.N, job.Cin, job.ntaps, job.tr, job.stem, dt, op(j))
        else:
            rows, pre = [], 0
            for j, job in enumerate(case.jobs):
                rows.append([wp(j), op(j), job.N, job.Cin, job.ntaps, job.tr | (job.stem << 1), pre, job.ld | (job.col << 32)])
                pre += job.numel
            rows.append([0, 0, 0, 0, 0, 0, pre, 0])
            table = side.put(torch.tensor(rows, dtype=torch.int64))
            with pack_tiled(side.api, 1 if path == "tiled" else 0):
                side.call("vinet_pack_weights_multi", table.data_ptr(), len(case.jobs), pre, dt)
            assert torch.equal(table.cpu(), torch.tensor(rows, dtype=torch.int64)), "%r: the job table changed" % case
        same_bits(out.cpu(), want, "%r %s %s" % (case, PDTN[dt], path))
        ran[path] = want.numel()
    same_bits(wdev.cpu(), warena, "%r: the weights" % case)
    return ran


def check_f32s_reference(case):
    """the F32S reference itself: de-permuting gives hi + lo within 2^-16 |v| of v, padding is zero, every position of a destination
    is written exactly once (the sentinel nowhere inside, nothing outside)"""
    want, _ = pack_expected(case, F32S)
    plain, _ = pack_expected(case, F32)
    dests_s, _ = _pack_layout(case, F32S)
    dests_p, _ = _pack_layout(case, F32)
    sent = torch.tensor(SENTINEL).bfloat16()
    inside = torch.zeros(want.numel(), dtype=torch.bool)
    for (key, members, off_s, n_s), (_, _, off_p, n_p) in zip(dests_s, dests_p):
        assert n_s == 2 * n_p
        inside[off_s:off_s + n_s] = True
        st, v = want[off_s:off_s + n_s].float().view(-1, 2, 32), plain[off_p:off_p + n_p].view(-1, 32)
        pos = torch.tensor(F32S_POS)
        hi, lo = st[:, 0, :][:, pos], st[:, 1, :][:, pos]            # channel c of a chunk sits at K position F32S_POS[c]
        written = v != SENTINEL
        if not case.jobs[members[0]].ld:
            assert bool(written.all()), "%r: a position of %r is not written" % (case, key)
        assert not bool(((hi == float(sent)) & written).any())
        assert bool((hi[~written] == float(sent)).all()) and bool((lo[~written] == float(sent)).all()), "%r: wrote outside its columns" % case
        err = ((hi + lo).double() - v.double()).abs()[written]
        assert bool((err <= 2.0 ** -16 * v.double().abs()[written]).all()), "%r: hi + lo is not v to 2^-16" % case
        assert bool((hi[written & (v == 0)] == 0).all()) and bool((lo[written & (v == 0)] == 0).all())
        # exactly once: F32S_POS is a permutation, so as many bf16 are written as twice the logical elements
        assert int((want[off_s:off_s + n_s] != sent).sum()) == 2 * int(written.sum())
    assert bool((want[~inside] == sent).all())
    # the permutation hits every position of a chunk once
    probe = torch.zeros(64, dtype=torch.bfloat16)
    encode_pack(torch.arange(1.0, 33.0), torch.ones(32, dtype=torch.bool), F32S, probe)
    assert sorted(probe[:32].tolist()) == [float(i) for i in range(1, 33)] and not bool(probe[32:].any())


def check_unpack(side, case, flags, paths=PACK_PATHS):
    G = 16
    jobs = case.jobs
    doff, goff, d, g = [], [], G, G
    for job in jobs:
        doff.append(d)
        goff.append(g)
        d += job.numel + G
        g += job.N * job.Cin * job.ntaps + G
    dw0, g0 = torch.full((d,), SENTINEL), torch.full((g,), SENTINEL)
    dwant, gwant = dw0.clone(), g0.clone()
    for j, job in enumerate(jobs):
        gen = _gen("unpack", case.tag, j)
        D = torch.randn((job.nsl, job.N, job.Kp), generator=gen)          # padding columns arrive non-zero
        old = torch.randn((job.N, job.Cin, job.ntaps), generator=gen)
        if job.stem:
            v = torch.zeros_like(old)
            for kh in range(7):
                for kw in range(7):
                    v[:, :, kh * 7 + kw] = D[kh, :, kw * 4:kw * 4 + job.Cin]
        else:
            v = D[:, :, :job.Cin].permute(1, 2, 0)
        dw0[doff[j]:doff[j] + job.numel] = D.reshape(-1)
        g0[goff[j]:goff[j] + old.numel()] = old.reshape(-1)
        dwant[doff[j]:doff[j] + job.numel] = 0.0 if flags & 2 else D.reshape(-1)
        gwant[goff[j]:goff[j] + old.numel()] = ((old + v) if flags & 1 else v).reshape(-1)
    assert float(dw0.abs().min()) > 0
    ran = {}
    for path in paths:
        if path == "single" and not case.single:
            continue
        dw, gr = side.put(dw0), side.put(g0)
        if path == "single":
            for j, job in enumerate(jobs):
                side.call("vinet_unpack_wgrad", dw.data_ptr() + 4 * doff[j], job.N, job.Cin, job.ntaps, job.stem, flags, gr.data_ptr() + 4 * goff[j])
        else:
            rows, pre = [], 0
            for j, job in enumerate(jobs):
                rows.append([dw.data_ptr() + 4 * doff[j], gr.data_ptr() + 4 * goff[j], job.N, job.Cin, job.ntaps, job.stem, pre, 0])
                pre += job.numel
            rows.append([0, 0, 0, 0, 0, 0, pre, 0])
            table = side.put(torch.tensor(rows, dtype=torch.int64))
            with pack_tiled(side.api, 1 if path == "tiled" else 0):
                side.call("vinet_unpack_wgrad_multi", table.data_ptr(), len(jobs), pre, flags)
            assert torch.equal(table.cpu(), torch.tensor(rows, dtype=torch.int64)), "%r: the job table changed" % case
        what = "%r flags %d %s" % (case, flags, path)
        same_bits(gr.cpu(), gwant, what + ": grad")
        same_bits(dw.cpu(), dwant, what + ": workspace")
        ran[path] = gwant.numel()
    return ran


# =====================================================================================================================
# vinet_import_ncdhw, vinet_import_ncdhw_pad, vinet_export_ncdhw
# =====================================================================================================================
# voxel counts 1, 255, 256, 257 and an extent of 1 in each of T, H, W (with two batch items)
IO_DIMS = ((1, 1, 1, 1), (1, 3, 5, 17), (2, 2, 8, 8), (1, 1, 1, 257), (2, 1, 5, 3), (2, 3, 1, 5), (2, 3, 5, 1))
FORMS = ("dense", "chan", "tslice", "both")
AFFS = ("none", "affine", "relu")          # nothing; scale + shift + relu; relu only
BLOCK = 256                                # voxels a block of the one-thread-per-voxel kernels owns


class ICase:
    """kind 'import' | 'import_pad' | 'export'.  dims: the channels-last view's (B, T, H, W); Cc: channels moved; dstC: the view's
    channels; src: 'perm' (a permuted [B,T,C,H,W] tensor: train.py) | 'bcast' (sc = st = 0: the decoder tail's map gradient);
    pad: (Hs, Ws, pad_top, pad_left); export: acc, aff, data, perm (the planar side as [C,B,T,H,W])"""

    def __init__(self, kind, dt, dims, Cc, dstC, form, src="perm", pad=None, acc=0, aff="none", data="exact", perm=False):
        self.kind, self.dt, self.dims, self.C, self.dstC, self.form, self.src, self.pad = kind, dt, dims, Cc, dstC, form, src, pad
        self.acc, self.aff, self.data, self.perm = acc, aff, data, perm
        self.id = "%s-%s-%s-c%d.%d-%s-%s%s" % (kind, DTN[dt], "x".join(map(str, dims)), Cc, dstC, form, src,
                                              "" if pad is None else "-pad%d.%d.%d.%d" % pad)
        if kind == "export":
            self.id = "export-%s-%s-c%d-%s-acc%d-%s-%s-%s" % (DTN[dt], "x".join(map(str, dims)), Cc, form, acc, aff, data, "perm" if perm else "ncdhw")

    def __repr__(self):
        return self.id


def _build_io():
    out, seen = [], set()

    def add(*a, **k):
        c = ICase(*a, **k)
        if c.id not in seen:
            seen.add(c.id)
            out.append(c)

    cd = ((1, 4), (3, 4), (4, 4), (5, 8), (3, 8), (4, 8), (1, 8))
    i = 0
    for dt in DTS:
        for dims in IO_DIMS:
            for Cc, dstC in cd:
                add("import", dt, dims, Cc, dstC, FORMS[i % 4], "bcast" if i % 5 == 4 else "perm")
                i += 1
            for form in FORMS:
                add("import", dt, dims, 3, 4, form)
        # import_pad: (dims of the padded view, Hs, Ws, pad_top, pad_left)
        pads = [((1, 1, 5, 7), 5, 7, 0, 0), ((2, 2, 9, 11), 3, 5, 3, 3), ((2, 2, 9, 11), 6, 6, 3, 5), ((1, 3, 4, 9), 4, 4, 0, 5),
                ((2, 1, 7, 9), 1, 1, 3, 3), ((1, 2, 1, 1), 1, 1, 0, 0), ((1, 1, 8, 6), 2, 1, 0, 5), ((2, 1, 5, 300), 2, 290, 3, 5),
                ((2, 2, 3 + 6, 5 + 8 + 1), 3, 5, 3, 3), ((2, 2, 4 + 6, 6 + 8), 4, 6, 3, 3), ((1, 1, 1 + 6, 1 + 8 + 1), 1, 1, 3, 3)]      # the folded stem
        for k, (dims, Hs, Ws, pt, pl) in enumerate(pads):
            for Cc, dstC in ((3, 4), (5, 8), (4, 4), (1, 4)):
                add("import_pad", dt, dims, Cc, dstC, FORMS[(k + Cc) % 4], "bcast" if (k + Cc) % 7 == 6 else "perm", pad=(Hs, Ws, pt, pl))
        for dims in IO_DIMS:
            for Cc in (4, 8):
                for data in ("exact", "rand"):
                    for acc in (0, 1):
                        for aff in AFFS:
                            add("export", dt, dims, Cc, Cc, FORMS[i % 4], acc=acc, aff=aff, data=data, perm=(i % 3 == 0))
                            i += 1
    return out


def _planar(case, gen):
    """(the planar fp32 base tensor, strides (sb, sc, st, sh, sw), its logical [B, C, T, Hs, Ws] view)"""
    B, T, H, W = case.dims
    Hs, Ws = (H, W) if case.pad is None else case.pad[:2]
    if case.src == "bcast":
        base = torch.randn((B, Hs, Ws), generator=gen)
        return base, (Hs * Ws, 0, 0, Ws, 1), base.view(B, 1, 1, Hs, Ws).expand(B, case.C, T, Hs, Ws)
    base = torch.randn((B, T, case.C, Hs, Ws), generator=gen)
    return base, (T * case.C * Hs * Ws, Hs * Ws, case.C * Hs * Ws, Ws, 1), base.permute(0, 2, 1, 3, 4)


def check_import(side, case):
    B, T, H, W = case.dims
    base, (sb, sc, st, sh, sw), logical = _planar(case, _gen("import", case.id))
    sdev = side.put(base)
    dims5 = case.dims + (case.dstC,)
    want = torch.zeros(dims5).to(TDT[case.dt])
    if case.pad is None:
        want[..., :case.C] = logical.permute(0, 2, 3, 4, 1).to(TDT[case.dt])
    else:
        Hs, Ws, pt, pl = case.pad
        want[:, :, pt:pt + Hs, pl:pl + Ws, :case.C] = logical.permute(0, 2, 3, 4, 1).to(TDT[case.dt])
    dst = Slab(dims5, case.dt, fill=SENTINEL, **view_geo(case.form, dims5, case.dstC))
    assert quad_ok(dst)
    db = put_tailed(side, dst, BLOCK, SENTINEL)
    if case.pad is None:
        side.call("vinet_import_ncdhw", sdev.data_ptr(), sb, sc, st, sh, sw, case.C, dst.ct(db), case.dt)
    else:
        side.call("vinet_import_ncdhw_pad", sdev.data_ptr(), sb, sc, st, sh, sw, case.C, *case.pad, dst.ct(db), case.dt)
    host = untailed(db, dst, SENTINEL, repr(case))
    dst.assert_outside_untouched(host, repr(case))
    n = same_bits(dst.inner(host).contiguous(), want, repr(case))
    same_bits(sdev.cpu(), base, "%r: the source" % case)
    return dict(elements=n)


def exact_affine(Cc, gen):
    return _pick([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], Cc, gen), torch.randint(-4, 5, (Cc,), generator=gen).float()


def rand_affine(Cc, gen):
    return (0.5 + torch.rand((Cc,), generator=gen)) * _pick([-1.0, 1.0], Cc, gen), 0.5 * torch.randn((Cc,), generator=gen)


def affine_ref(x, aff, scale, shift, old, wide):
    """(reference, bound) of relu?(x * scale + shift) + old in float64 (wide) or in fp32 (exact data: every step is exact there)"""
    tp = torch.float64 if wide else torch.float32
    t = x.to(tp)
    mag = t.abs()
    if aff == "affine":
        mag = (t * scale.to(tp)).abs() + shift.to(tp).abs()
        t = t * scale.to(tp) + shift.to(tp)
    if aff != "none":
        t = torch.where(t > 0, t, torch.zeros((), dtype=tp))
    if old is not None:
        t, mag = t + old.to(tp), mag + old.to(tp).abs()
    return t, 2 * U32 * mag


def assert_exact(ref, what):
    assert torch.equal((ref * 2).round(), ref * 2) and float(ref.abs().max()) <= 18 and not bool(((ref == 0) & torch.signbit(ref)).any()), what + ": not exact data"
    assert torch.equal(ref.bfloat16().to(ref.dtype), ref), what


def gate_affine(got, ref, bound, data, ddt, what):
    """bit equality on exact data; the derived bound (plus half a bf16 ulp for a bf16 destination) on random data"""
    if data == "exact":
        assert_exact(ref, what)
        return dict(elements=same_bits(got.contiguous(), ref.to(TDT[ddt]).contiguous(), what))
    if ddt == BF16:
        bound = bound + bf16_half_ulp(ref.abs() + bound)
    return dict(err_over_bound=gate_bound(got, ref, bound, what))


def _draw(shape, data, gen, lim):
    return torch.randint(-lim, lim + 1, shape, generator=gen).float() if data == "exact" else torch.randn(shape, generator=gen)


def check_export(side, case):
    B, T, H, W = case.dims
    Cc = case.C
    gen = _gen("export", case.id)
    dims5 = case.dims + (Cc,)
    xv = _draw(dims5, case.data, gen, 3).to(TDT[case.dt])
    scale, shift = exact_affine(Cc, gen) if case.data == "exact" else rand_affine(Cc, gen)
    src = Slab(dims5, case.dt, fill=NAN, values=xv, **view_geo(case.form, dims5, Cc))
    xb = put_tailed(side, src, BLOCK, NAN)
    # the planar side: channels [1, C + 1) of a [B, C + 2, T, H, W] tensor (or [C + 2, B, T, H, W]), the sentinel everywhere else
    shape = (Cc + 2, B, T, H, W) if case.perm else (B, Cc + 2, T, H, W)
    full = torch.full(shape, SENTINEL)
    inner = (full[1:Cc + 1].permute(1, 2, 3, 4, 0) if case.perm else full[:, 1:Cc + 1].permute(0, 2, 3, 4, 1))        # [B, T, H, W, C] view
    old = _draw(dims5, case.data, gen, 8) if case.acc else None
    if case.acc:
        inner.copy_(old)
    before = full.clone()
    vs, vh = Vec(side, scale, 4), Vec(side, shift, 4)
    pre = L.CAffine(vs.ptr, vh.ptr, 1) if case.aff == "affine" else L.CAffine(None, None, 1 if case.aff == "relu" else 0)
    ddev = side.put(torch.cat([full.reshape(-1), torch.full((BLOCK * (Cc + 2),), SENTINEL)]))
    n1 = T * H * W
    sb, sc = (n1, B * n1) if case.perm else ((Cc + 2) * n1, n1)
    first = (B * n1 if case.perm else n1) * 4            # byte offset of channel 1
    side.call("vinet_export_ncdhw", src.ct(xb), case.dt, pre, ddev.data_ptr() + first, sb, sc, H * W, W, 1, case.acc)
    got_all = ddev.cpu()
    assert bool((got_all[full.numel():] == SENTINEL).all()), "%r: wrote behind the end of its buffer" % case
    got_full = got_all[:full.numel()].view(shape)
    got = (got_full[1:Cc + 1].permute(1, 2, 3, 4, 0) if case.perm else got_full[:, 1:Cc + 1].permute(0, 2, 3, 4, 1))
    outside = torch.ones(shape, dtype=torch.bool)
    if case.perm:
        outside[1:Cc + 1] = False
    else:
        outside[:, 1:Cc + 1] = False
    assert torch.equal(_bits(got_full[outside]), _bits(before[outside])), "%r: wrote outside its channels" % case
    ref, bound = affine_ref(xv, case.aff, scale, shift, old, case.data != "exact")
    errs = gate_affine(got, ref, bound, case.data, F32, repr(case))
    same_bits(untailed(xb, src, NAN, "%r: source" % case), src.base, "%r: the source" % case)
    return errs


IO_CASES = _build_io()
IMPORT_CASES = [c for c in IO_CASES if c.kind != "export"]
EXPORT_CASES = [c for c in IO_CASES if c.kind == "export"]


# =====================================================================================================================
# vinet_copy_affine, vinet_split_bf16
# =====================================================================================================================
OCT_MIN = 65536


def copy_vb(Cc):
    """voxels per block of copy_affine8_kernel below 16 384 blocks"""
    return 16 * (256 // min(Cc // 8, 256))


def copy_route(sdt, ddt, src, dst, nvox):
    """the kernel vinet_copy_affine launches for these Slabs"""
    if sdt == BF16 and ddt == BF16 and oct_ok(src) and oct_ok(dst) and nvox >= OCT_MIN:
        return "copy_affine8_kernel"
    return "copy_affine_kernel<%s,%s>" % (DTN[sdt], DTN[ddt])


class Geo:
    """the numbers of a Slab without its buffer (the routes are worked out for every case when the tables are built)"""

    def __init__(self, dims, dt, ld=None, c_off=0, t_total=None, t_off=0, **unused):
        B, T, H, W, Cc = dims
        self.dims, self.dt, self.ld = dims, dt, Cc if ld is None else ld
        self.sB = (T if t_total is None else t_total) * H * W * self.ld
        self.off = t_off * H * W * self.ld + c_off


def make_slab(dims, dt, form, chan=None, cls=Slab, **kw):
    """a Slab (or Geo) of a view form.  'sB_plus4' (beside bn_cases' forms): dense rows and an aligned pointer, batch items 4 elements
    further apart than their voxels need -- sB % 8 == 4 and nothing else off the 8-channel grid; the buffer keeps one spare frame
    per batch item for it"""
    if form != "sB_plus4":
        return cls(dims, dt, **kw, **view_geo(form, dims, dims[4], chan))
    values = kw.pop("values", None)
    s = cls(dims, dt, t_total=dims[1] + 1, **kw)
    s.sB = dims[1] * dims[2] * dims[3] * s.ld + 4
    if values is not None:          # (after the batch stride has moved)
        s.inner(s.base).copy_(values.to(TDT[dt]))
    return s


def oct_failures(g):
    """which conditions of csrc/elementwise.h oct_ok a Slab or Geo fails"""
    es = 4 if g.dt == F32 else 2
    return [n for n, bad in (("C", g.dims[4] % 8), ("ld", g.ld % 8), ("sB", g.sB % 8), ("ptr", (g.off * es) % 16)) if bad]


class CCase:
    """dform 'inplace': the destination is the source's view (materialise); else a view form of its own buffer (concat).
    schan / dchan: (ld, c_off) of a channel slice"""

    def __init__(self, tag, sdt, ddt, nvox, Cc, data, acc=0, aff="none", sform="dense", dform="dense", schan=None, dchan=None):
        self.tag, self.sdt, self.ddt, self.nvox, self.C, self.data, self.acc, self.aff = tag, sdt, ddt, nvox, Cc, data, acc, aff
        self.sform, self.dform, self.schan, self.dchan = sform, dform, schan, dchan
        self.dims = dims_of(nvox) + (Cc,)
        s = make_slab(self.dims, sdt, sform, schan, Geo)
        d = s if dform == "inplace" else make_slab(self.dims, ddt, dform, dchan, Geo)
        assert quad_ok(s) and quad_ok(d) and (dform != "inplace" or sdt == ddt), tag
        self.kernel = copy_route(sdt, ddt, s, d, nvox)
        self.id = "%s-%s_%s-v%d-c%d-%s-acc%d-%s-s_%s%s-d_%s%s" % (tag, DTN[sdt], DTN[ddt], nvox, Cc, data, acc, aff, sform, "" if schan is None else "%d.%d" % schan,
                                                               dform, "" if dchan is None else "%d.%d" % dchan)

    def slabs(self, fill, xv=None, old=None):
        s = make_slab(self.dims, self.sdt, self.sform, self.schan, fill=NAN if fill is None else fill, values=xv)
        if self.dform == "inplace":
            return s, s
        return s, make_slab(self.dims, self.ddt, self.dform, self.dchan, fill=SENTINEL if fill is None else fill, values=old)

    def __repr__(self):
        return self.id


def _build_copy():
    out, seen = [], set()

    def add(*a, **k):
        c = CCase(*a, **k)
        if c.id not in seen:
            seen.add(c.id)
            out.append(c)
        return c

    # the quad kernel: four type pairs x accumulate x three affine forms at 1, 255, 256, 257 quads (C = 4) and 3, 255, 258 (C = 12)
    i = 0
    for sdt in DTS:
        for ddt in DTS:
            for acc in (0, 1):
                for aff in AFFS:
                    for Cc, nvox in ((4, 1), (4, 255), (4, 256), (4, 257), (12, 1), (12, 85), (12, 86)):
                        for data in ("exact", "rand"):
                            sform, dform = FORMS[i % 4], FORMS[(i // 4 + 1) % 4]
                            if sdt == ddt and i % 7 == 3:
                                dform = "inplace"
                            add("quad", sdt, ddt, nvox, Cc, data, acc, aff, sform, dform)
                        i += 1
    # at 65 536 voxels, bf16 to bf16, 8 channels: off the 8-channel grid for one reason alone (bn_cases' sB4mod8 form: ld = 12 and the pointer
    # with it), on either side and in place
    off_grid = (("ptr8mod16", "chan", (16, 4)), ("ld_c_plus4", "chan", (12, 0)), ("sB4mod8", "both", (12, 4)), ("sB_alone", "sB_plus4", None))
    for k, (tag, form, chan) in enumerate(off_grid):
        for data in ("exact", "rand"):
            add(tag, BF16, BF16, OCT_MIN, 8, data, k % 2, AFFS[k % 3], form, "dense", schan=chan)
            add(tag, BF16, BF16, OCT_MIN, 8, data, 1 - k % 2, AFFS[(k + 1) % 3], "dense", form, dchan=chan)
            add(tag, BF16, BF16, OCT_MIN, 8, data, k % 2, AFFS[(k + 2) % 3], form, "inplace", schan=chan)
    # the route threshold and the block seam of the 8-channel kernel
    i = 0
    for Cc in (8, 24, 200):
        vb = copy_vb(Cc)
        for nvox in (OCT_MIN - 1, OCT_MIN, OCT_MIN + 1, OCT_MIN + vb - 1, OCT_MIN + vb + 1):
            pairs = (("inplace", FORMS[i % 4]), (("chan", "both")[i % 2], ("dense", "tslice", "chan")[i % 3]))
            if Cc == 200:          # (a T slice of 13 M elements triples its buffer: the wide cases stay dense or channel-sliced)
                pairs = (("inplace", ("dense", "chan")[i % 2]), ("chan", ("dense", "chan")[(i // 2) % 2]))
            for dform, sform in pairs:
                for data in (("exact", "rand") if Cc <= 24 else ("exact",)):
                    add("seam", BF16, BF16, nvox, Cc, data, i % 2, AFFS[i % 3], sform, dform)
                i += 1
    add("seam", BF16, BF16, OCT_MIN, 512, "exact", 1, "affine", "dense", "inplace")
    # the other type pairs stay on the quad kernel past the threshold
    for sdt, ddt in ((F32, F32), (F32, BF16), (BF16, F32)):
        add("pairs", sdt, ddt, OCT_MIN, 8, "exact", 1, "affine", "dense", "chan")
    return out


@functools.lru_cache(maxsize=8)
def _copy_data(dims, sdt, ddt, data):
    """(x in the source type, the old destination in its type, scale, shift); shared by the cases of a shape, never changed"""
    gen = _gen("copy", dims, sdt, ddt, data)
    scale, shift = exact_affine(dims[4], gen) if data == "exact" else rand_affine(dims[4], gen)
    return _draw(dims, data, gen, 3).to(TDT[sdt]), _draw(dims, data, gen, 8).to(TDT[ddt]), scale, shift


def check_copy(side, case):
    xv, oldv, scale, shift = _copy_data(case.dims, case.sdt, case.ddt, case.data)
    inplace = case.dform == "inplace"
    old = (xv if inplace else oldv) if case.acc else None
    src, dst = case.slabs(None, xv, old)
    over = copy_vb(case.C) if case.kernel == "copy_affine8_kernel" else BLOCK
    sb = put_tailed(side, src, over, SENTINEL if inplace else NAN)
    db = sb if inplace else put_tailed(side, dst, over, SENTINEL)
    vs, vh = Vec(side, scale, 4), Vec(side, shift, 4)
    pre = L.CAffine(vs.ptr, vh.ptr, 1) if case.aff == "affine" else L.CAffine(None, None, 1 if case.aff == "relu" else 0)
    side.call("vinet_copy_affine", src.ct(sb), case.sdt, pre, dst.ct(db), case.ddt, case.acc)
    host = untailed(db, dst, SENTINEL, repr(case))
    dst.assert_outside_untouched(host, repr(case))
    ref, bound = affine_ref(xv, case.aff, scale, shift, old, case.data != "exact")
    errs = gate_affine(dst.inner(host), ref, bound, case.data, case.ddt, repr(case))
    if not inplace:
        same_bits(untailed(sb, src, NAN, "%r: source" % case), src.base, "%r: the source" % case)
    return errs


# (quads, hi form, lo form, hi chan, lo chan): planes with different ld, one of them a T slice
SPLIT_SHAPES = ((1, "chan", "tslice", (12, 4), None), (255, "tslice", "chan", None, (8, 4)), (257, "both", "dense", (20, 8), None),
                (255, "dense", "both", None, (12, 4)))
SPLIT_DIMS = {1: (1, 1, 1, 1), 255: (1, 3, 5, 17), 257: (1, 1, 1, 257)}
SPLIT_CASES = [(q, hf, lf, hc, lc, aff, data, sform) for k, (q, hf, lf, hc, lc) in enumerate(SPLIT_SHAPES) for aff in AFFS for data in ("exact", "rand")
               for sform in (FORMS[k % 4],)]


def check_split(side, quads, hform, lform, hchan, lchan, aff, data, sform):
    dims = SPLIT_DIMS[quads] + (4,)
    what = "split q%d %s %s %s" % (quads, aff, data, sform)
    gen = _gen("split", quads, aff, data)
    xv = _draw(dims, data, gen, 3)
    scale, shift = exact_affine(4, gen) if data == "exact" else rand_affine(4, gen)
    src = Slab(dims, F32, fill=NAN, values=xv, **view_geo(sform, dims, 4))
    hi = Slab(dims, BF16, fill=SENTINEL, **view_geo(hform, dims, 4, hchan))
    lo = Slab(dims, BF16, fill=SENTINEL, **view_geo(lform, dims, 4, lchan))
    assert quad_ok(src) and quad_ok(hi) and quad_ok(lo) and hi.ld != lo.ld
    sb, hb, lb = put_tailed(side, src, BLOCK, NAN), put_tailed(side, hi, BLOCK, SENTINEL), put_tailed(side, lo, BLOCK, SENTINEL)
    vs, vh = Vec(side, scale, 4), Vec(side, shift, 4)
    pre = L.CAffine(vs.ptr, vh.ptr, 1) if aff == "affine" else L.CAffine(None, None, 1 if aff == "relu" else 0)
    side.call("vinet_split_bf16", src.ct(sb), pre, hi.ct(hb), lo.ct(lb))
    planes = []
    for slab, buf, nm in ((hi, hb, "hi"), (lo, lb, "lo")):
        host = untailed(buf, slab, SENTINEL, what + ": " + nm)
        slab.assert_outside_untouched(host, what + ": " + nm)
        planes.append(slab.inner(host).contiguous())
    same_bits(untailed(sb, src, NAN, what + ": source"), src.base, what + ": the source")
    ref, bound = affine_ref(xv, aff, scale, shift, None, data != "exact")
    if data == "exact" or aff != "affine":
        if data == "exact":
            assert_exact(ref, what)
        v = ref.float()
        assert torch.equal(v.double(), ref.double())              # (relu only / no affine: the fp32 input itself)
        n = same_bits(planes[0], v.bfloat16(), what + ": hi")
        return dict(elements=n + same_bits(planes[1], (v - v.bfloat16().float()).bfloat16(), what + ": lo"))
    rec = planes[0].double() + planes[1].double()
    return dict(rec_over_bound=gate_bound(rec, ref, bound + 2.0 ** -16 * (ref.abs() + bound), what + ": hi + lo"))


COPY_CASES = _build_copy()
COPY_KERNELS = ("copy_affine_kernel<f32,f32>", "copy_affine_kernel<f32,bf16>", "copy_affine_kernel<bf16,f32>", "copy_affine_kernel<bf16,bf16>",
                "copy_affine8_kernel")


# =====================================================================================================================
# refusals: the return value and the message only -- a refused call launches nothing
# =====================================================================================================================
def _refused(side, needle, fn, *args):
    rc = getattr(side.api, fn)(*args, side.stream)
    assert rc != 0, fn + " accepted what it has to refuse"
    assert needle in side.api.vinet_last_error(), (fn, side.api.vinet_last_error())


def check_refusals(side):
    none = L.CAffine(None, None, 0)
    dims = (1, 2, 3, 5, 8)
    mk = lambda dt, **k: Slab(dims, dt, fill=3.0, **k)
    good, good16 = mk(F32), mk(BF16)
    gb, gb16 = side.put(good.base), side.put(good16.base)
    plane = side.put(torch.full((2 * 8 * 3 * 5 + 8,), 3.0))
    st = (8 * 15, 15, 8 * 15, 5, 1)

    def bad_views():
        """views failing quad_ok: C % 4, ld % 4, sB % 4, a pointer off the 4-element grid"""
        c6 = Slab((1, 2, 3, 5, 6), F32, fill=3.0, ld=8)
        ld10 = Slab((1, 2, 3, 5, 8), F32, fill=3.0, ld=10)
        sb2 = mk(F32)
        sb2.sB += 2
        off2 = mk(F32, ld=12, c_off=2)
        return [c6, ld10, sb2, off2]

    for v in bad_views():
        vb = side.put(torch.cat([v.base, torch.full((64,), 3.0)]))
        _refused(side, b"import_ncdhw: bad arguments", "vinet_import_ncdhw", plane.data_ptr(), *st, 3, v.ct(vb), F32)
        _refused(side, b"import_ncdhw_pad: bad arguments", "vinet_import_ncdhw_pad", plane.data_ptr(), *st, 3, 1, 1, 0, 0, v.ct(vb), F32)
        _refused(side, b"export_ncdhw: bad arguments", "vinet_export_ncdhw", v.ct(vb), F32, none, plane.data_ptr(), *st, 0)
        _refused(side, b"copy_affine: bad views", "vinet_copy_affine", v.ct(vb), F32, none, good.ct(gb), F32, 0)
        _refused(side, b"copy_affine: bad views", "vinet_copy_affine", good.ct(gb), F32, none, v.ct(vb), F32, 0)
        _refused(side, b"split_bf16: bad views", "vinet_split_bf16", v.ct(vb), none, good16.ct(gb16), good16.ct(gb16))
        assert bool((vb.cpu() == 3.0).all())
    # mismatched dims
    other = Slab((1, 2, 3, 4, 8), F32, fill=3.0)
    ob = side.put(other.base)
    other16 = Slab((1, 2, 3, 5, 12), BF16, fill=3.0)
    ob16 = side.put(other16.base)
    _refused(side, b"copy_affine: bad views", "vinet_copy_affine", good.ct(gb), F32, none, other.ct(ob), F32, 0)
    _refused(side, b"split_bf16: bad views", "vinet_split_bf16", good.ct(gb), none, other16.ct(ob16), good16.ct(gb16))
    _refused(side, b"split_bf16: bad views", "vinet_split_bf16", good.ct(gb), none, good16.ct(gb16), other16.ct(ob16))
    # C > dst.C, C = 0; pads past the destination; an empty source
    _refused(side, b"import_ncdhw: bad arguments", "vinet_import_ncdhw", plane.data_ptr(), *st, 9, good.ct(gb), F32)
    _refused(side, b"import_ncdhw: bad arguments", "vinet_import_ncdhw", plane.data_ptr(), *st, 0, good.ct(gb), F32)
    _refused(side, b"import_ncdhw_pad: bad arguments", "vinet_import_ncdhw_pad", plane.data_ptr(), *st, 9, 3, 5, 0, 0, good.ct(gb), F32)
    for Hs, Ws, pt, pl in ((3, 5, 1, 0), (3, 5, 0, 1), (2, 2, 2, 0), (2, 2, 0, 4), (0, 5, 0, 0), (3, 0, 0, 0), (1, 1, -1, 0), (1, 1, 0, -1)):
        _refused(side, b"import_ncdhw_pad: bad arguments", "vinet_import_ncdhw_pad", plane.data_ptr(), *st, 3, Hs, Ws, pt, pl, good.ct(gb), F32)
    # packing: a bad dtype, stems that are no 1 x 7 x 7 over at most 4 channels, empty tables
    w, out = side.put(torch.full((64 * 5 * 49,), 3.0)), side.put(torch.full((7 * 64 * 64,), 3.0))
    _refused(side, b"pack_weights: bad dtype", "vinet_pack_weights", w.data_ptr(), 4, 4, 1, 0, 0, 3, out.data_ptr())
    _refused(side, b"pack_weights: bad dtype", "vinet_pack_weights", w.data_ptr(), 4, 4, 1, 0, 0, -1, out.data_ptr())
    for N, Cin, nt, tr in ((64, 3, 48, 0), (64, 3, 50, 0), (64, 5, 49, 0), (64, 3, 49, 1)):
        _refused(side, b"pack_weights stem", "vinet_pack_weights", w.data_ptr(), N, Cin, nt, tr, 1, F32, out.data_ptr())
    _refused(side, b"pack_weights: bad arguments", "vinet_pack_weights", w.data_ptr(), 0, 4, 1, 0, 0, F32, out.data_ptr())
    table = side.put(torch.tensor([[w.data_ptr(), out.data_ptr(), 4, 4, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0, 128, 0]], dtype=torch.int64))
    _refused(side, b"pack_weights_multi: bad arguments", "vinet_pack_weights_multi", table.data_ptr(), 0, 128, F32)
    _refused(side, b"pack_weights_multi: bad arguments", "vinet_pack_weights_multi", table.data_ptr(), 1, 0, F32)
    _refused(side, b"unpack_wgrad_multi: bad arguments", "vinet_unpack_wgrad_multi", table.data_ptr(), 0, 128, 3)
    _refused(side, b"unpack_wgrad: bad arguments", "vinet_unpack_wgrad", out.data_ptr(), 4, 0, 1, 0, 3, w.data_ptr())
    for buf in (gb, gb16, plane, ob, ob16, w, out):
        assert bool((buf.cpu() == 3.0).all()), "a refused call wrote something"
