// The message layer between time slabs: event-ordered peer copies, pull launches and RCCL groups behind shift(), the
// second-stream bracket (solver.h: comm_z), halo / tail exchanges of the loop, slab <-> pencil transposes and the
// partitioned tridiagonal t-solve (tri.hip).  Host code only.
#include "solver.h"

#include "comm.h"

namespace dotsocp {

// The slab's next ordering event (round-robin; a wait captures the record that precedes it, so reuse is safe)
static hipEvent_t next_xev(Slab &s) {
    hipEvent_t e = s.ev[EV_X0 + s.xev_next];
    s.xev_next = (s.xev_next + 1) % DS_XEV;
    return e;
}

int Solver::xcopy(Slab &from, const double *src, Slab &to, double *dst, i64 count) {
    if (count <= 0) return 0;
    const size_t bytes = sizeof(double) * (size_t)count;
    DS_CHECK(comm_enter());
    const hipStream_t fs = cst(from), ts = cst(to);
    if (fs == ts) {
        DS_CHECK(use(to));
        DS_HIP(ds_memcpy_async(dst, src, bytes, hipMemcpyDeviceToDevice, ts));
        return comm_leave();
    }
    hipEvent_t a = next_xev(from), b = next_xev(to);
    DS_CHECK(use(from));
    DS_HIP(ds_event_record(a, fs));
    DS_CHECK(use(to));
    DS_HIP(ds_stream_wait_event(ts, a, 0));
    if (from.dev == to.dev) DS_HIP(ds_memcpy_async(dst, src, bytes, hipMemcpyDeviceToDevice, ts));
    else DS_HIP(ds_memcpy_peer_async(dst, to.dev, src, from.dev, bytes, ts));
    DS_HIP(ds_event_record(b, ts));
    DS_CHECK(use(from));
    DS_HIP(ds_stream_wait_event(fs, b, 0));
    return comm_leave();
}

int Solver::xcopy2d(Slab &from, const double *src, size_t spitch, Slab &to, double *dst, size_t dpitch, size_t width,
                    size_t height) {
    if (width == 0 || height == 0) return 0;
    DS_CHECK(comm_enter());
    const hipStream_t fs = cst(from), ts = cst(to);
    if (fs == ts) {
        DS_CHECK(use(to));
        DS_HIP(ds_memcpy2d_async(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice, ts));
        return comm_leave();
    }
    hipEvent_t a = next_xev(from), b = next_xev(to);
    DS_CHECK(use(from));
    DS_HIP(ds_event_record(a, fs));
    DS_CHECK(use(to));
    DS_HIP(ds_stream_wait_event(ts, a, 0));
    if (from.dev == to.dev || peer_ok) {
        // different devices: peer access was enabled in both directions when the slabs were placed (alloc_slabs)
        DS_HIP(ds_memcpy2d_async(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice, ts));
    } else {
        // peer access refused: row by row through hipMemcpyPeerAsync, which stages through the host by itself
        for (size_t r = 0; r < height; ++r)
            DS_HIP(ds_memcpy_peer_async((char *)dst + r * dpitch, to.dev, (const char *)src + r * spitch, from.dev, width, ts));
    }
    DS_HIP(ds_event_record(b, ts));
    DS_CHECK(use(from));
    DS_HIP(ds_stream_wait_event(fs, b, 0));
    return comm_leave();
}

// ---- communication on the second streams (solver.h: comm_z) ----
// (slabs that share a pair of streams -- dotsocp_create(.., nslabs) -- are served by the first of them)
int Solver::comm_fork() {
    if (!comm_z) return 0;
    FOR_SLABS(s) {
        if (&s != &slabs[0] && s.st == slabs[0].st) continue;
        DS_HIP(ds_event_record(s.ev[EV_FORK], s.st));
        DS_HIP(ds_stream_wait_event(s.st_z, s.ev[EV_FORK], 0));
    }
    return 0;
}

int Solver::comm_mark(SlabEvent ev) {
    if (!comm_z) return 0;
    FOR_SLABS(s) {
        if (&s != &slabs[0] && s.st == slabs[0].st) continue;
        DS_HIP(ds_event_record(s.ev[ev], s.st_z));
    }
    return 0;
}

int Solver::comm_wait(SlabEvent ev) {
    if (!comm_z) return 0;
    FOR_SLABS(s) {
        if (&s != &slabs[0] && s.st == slabs[0].st) continue;
        DS_HIP(ds_stream_wait_event(s.st, s.ev[ev], 0));
    }
    return 0;
}

int Solver::comm_enter() {
    if (!comm_z || comm_async) return 0;
    if (comm_depth++ == 0) DS_CHECK(comm_fork());
    return 0;
}

int Solver::comm_leave() {
    if (!comm_z || comm_async) return 0;
    if (--comm_depth == 0) {
        DS_CHECK(comm_mark(EV_CJOIN));
        DS_CHECK(comm_wait(EV_CJOIN));
    }
    return 0;
}

// --------------------------------------------------------------------------------------
// neighbour exchanges
// --------------------------------------------------------------------------------------
int Solver::shift(int dir, const Sel &src, const Sel &dst, i64 count) {
    if (!multi() || count <= 0) return 0;
    DS_CHECK(comm_enter());
    if (!remote()) {
        if (msg_batching()) {
            for (size_t i = 0; i + 1 < slabs.size(); ++i) {
                const int f = (int)((dir > 0) ? i : i + 1), t = (int)((dir > 0) ? i + 1 : i);
                msgs.push_back(Msg{f, t, src(slabs[f]), dst(slabs[t]), count});
            }
            if (msg_depth == 0) DS_CHECK(flush_msgs());       // a lone shift() is a group of one
            return comm_leave();
        }
        for (size_t i = 0; i + 1 < slabs.size(); ++i) {
            Slab &from = (dir > 0) ? slabs[i] : slabs[i + 1];
            Slab &to = (dir > 0) ? slabs[i + 1] : slabs[i];
            DS_CHECK(xcopy(from, src(from), to, dst(to), count));
        }
        return comm_leave();
    }
    Rccl &api = rccl_api();
    Slab &s = slabs[0];
    const hipStream_t cs = cst(s);
    const int to = rank + dir, from = rank - dir;
    DS_NCCL(api.GroupStart());
    ++open_groups;
    if (to >= 0 && to < world) DS_NCCL_G(api.Send(src(s), (size_t)count, ncclDouble, to, (ncclComm_t)nccl, cs));
    if (from >= 0 && from < world) DS_NCCL_G(api.Recv(dst(s), (size_t)count, ncclDouble, from, (ncclComm_t)nccl, cs));
    --open_groups;
    DS_NCCL(api.GroupEnd());
    return comm_leave();
}

int Solver::shift_edge_halo(const Sel &base) {
    if (!multi()) return 0;
    DS_CHECK(shift(-1, [&](Slab &s) { return base(s) + s.g.offBx; },
                   [&](Slab &s) { return base(s) + s.g.offBx + s.g.bxLayer * s.g.ntl; }, slabs[0].g.bxLayer));
    DS_CHECK(shift(-1, [&](Slab &s) { return base(s) + s.g.offBy; },
                   [&](Slab &s) { return base(s) + s.g.offBy + s.g.byLayer * s.g.ntl; }, slabs[0].g.byLayer));
    return 0;
}

// Several shift() calls issued as ONE RCCL group (nested groups are legal): traffic to the left and
// to the right neighbour then shares the bidirectional links instead of queueing behind each other.
int Solver::group_begin() {
    DS_CHECK(comm_enter());
    if (remote()) {
        DS_NCCL(rccl_api().GroupStart());
        ++open_groups;
    } else {
        ++msg_depth;
    }
    return 0;
}

int Solver::group_end() {
    if (remote()) {
        --open_groups;
        DS_NCCL(rccl_api().GroupEnd());
    } else if (--msg_depth == 0) {
        DS_CHECK(flush_msgs());
    }
    return comm_leave();
}

// Pull launches (a kernel on the receiver's device reading the sender's memory through a peer pointer): the default
// between slabs of ONE device.  Between different devices the event-ordered hipMemcpyPeerAsync copies are the default
// and the pull launches are opt-in (DOTSOCP_MSG_BATCH=1 / DOTSOCP_TRI_GATHER=1): whether the reading device's L2
// returns fresh lines of another device's coarse-grained memory behind nothing but an event wait has never been
// observed on two devices (the build's boxes have one).
bool Solver::pull_default(const char *var) const {
    const char *e = getenv(var);                                  // read per call: the tests switch it inside one process
    if (!peer_ok) return false;
    if (e) return atoi(e) != 0;
    return !cross_device;
}

bool Solver::msg_batching() const { return pull_default("DOTSOCP_MSG_BATCH"); }

// The collected copies of a group, as the event-ordered copies of xcopy() would do them but with one set of events and
// one launch per slab: every sender records "written", every receiver waits for its senders, pulls all its messages
// with one launch (peer pointers) and records "pulled", every sender waits for its receivers (its buffers are free).
int Solver::flush_msgs() {
    if (msgs.empty()) return 0;
    const size_t P = slabs.size();
    std::vector<char> sends(P, 0), gets(P, 0);
    for (const Msg &m : msgs)
        if (m.count > 0) { sends[m.from] = 1; gets[m.to] = 1; }
    for (size_t i = 0; i < P; ++i)
        if (sends[i]) {
            bool other = false;
            for (const Msg &m : msgs) other = other || (m.from == (int)i && m.count > 0 && cst(slabs[m.to]) != cst(slabs[i]));
            if (!other) continue;
            DS_CHECK(use(slabs[i]));
            DS_HIP(ds_event_record(slabs[i].ev[EV_MSG], cst(slabs[i])));
        }
    for (size_t t = 0; t < P; ++t) {
        if (!gets[t]) continue;
        Slab &to = slabs[t];
        DS_CHECK(use(to));
        GatherMsgs g{};
        g.n = 0;
        std::vector<char> waited(P, 0);
        for (const Msg &m : msgs) {
            if (m.to != (int)t || m.count <= 0) continue;
            if (!waited[m.from] && cst(slabs[m.from]) != cst(to)) {
                DS_HIP(ds_stream_wait_event(cst(to), slabs[m.from].ev[EV_MSG], 0));
                waited[m.from] = 1;
            }
            if (g.n == DS_MAX_WORLD) {
                DS_CHECK(launch_gather_msgs(g, cst(to)));
                g.n = 0;
            }
            g.src[g.n] = m.src; g.dst[g.n] = m.dst; g.count[g.n] = m.count;
            ++g.n;
        }
        DS_CHECK(launch_gather_msgs(g, cst(to)));
        bool other = false;
        for (const Msg &m : msgs) other = other || (m.to == (int)t && m.count > 0 && cst(slabs[m.from]) != cst(to));
        if (other) DS_HIP(ds_event_record(to.ev[EV_GOT], cst(to)));
    }
    for (size_t f = 0; f < P; ++f) {
        if (!sends[f]) continue;
        Slab &from = slabs[f];
        DS_CHECK(use(from));
        std::vector<char> waited(P, 0);
        for (const Msg &m : msgs)
            if (m.from == (int)f && m.count > 0 && !waited[m.to] && cst(slabs[m.to]) != cst(from)) {
                DS_HIP(ds_stream_wait_event(cst(from), slabs[m.to].ev[EV_GOT], 0));
                waited[m.to] = 1;
            }
    }
    msgs.clear();
    return 0;
}

// u0 = w.*q0 - alpha0 of every slab's last cell layer -> right neighbour (first node layer of its rhs)
int Solver::make_u0_tail() {
    if (!multi() || u0_made) return 0;        // (u0_made: the q-step wrote it)
    for (auto &s : slabs)
        if (!s.g.last) {
            DS_CHECK(use(s));
            DS_CHECK(launch_u0_tail(s.g, s.q, s.alpha, s.weight, s.send_plane, s.st));
        }
    return 0;
}

// (make_u0_tail() first: its kernel runs on the main streams)
int Solver::exchange_u0_tail() {
    if (!multi()) return 0;
    DS_CHECK(shift(+1, [](Slab &s) { return s.send_plane; }, [](Slab &s) { return s.u0_prev; }, slabs[0].g.plane));
    u0_fresh = true;
    return 0;
}

// first owned bx / by layers of every slab -> halo layer of its left neighbour; with_u0: the u0 tail
// of the new iterate travels to the right in the same group
int Solver::exchange_q_halo(bool with_u0) {
    if (!multi()) return 0;
    if (with_u0 && !comm_async) DS_CHECK(make_u0_tail());     // (an asynchronous caller has run it before its fork)
    prof_begin(PH_COMM, comm_z);
    const i64 bxL = slabs[0].g.bxLayer, byL = slabs[0].g.byLayer;
    DS_CHECK(group_begin());
    DS_CHECK(shift(-1, [](Slab &s) { return s.q + s.g.offBx; },
                   [](Slab &s) { return s.q + s.g.offBx + s.g.bxLayer * s.g.ntl; }, bxL));
    DS_CHECK(shift(-1, [](Slab &s) { return s.q + s.g.offBy; },
                   [](Slab &s) { return s.q + s.g.offBy + s.g.byLayer * s.g.ntl; }, byL));
    if (with_u0) DS_CHECK(exchange_u0_tail());
    DS_CHECK(group_end());
    prof_end(PH_COMM, comm_z);
    return 0;
}

int Solver::ensure_halo() {
    if (!halo_pending) return 0;
    halo_pending = false;
    return exchange_q_halo(true);
}

// slabs [y][x][t_local] <-> pencils [columns l0..l0+nl)[all t]; data in w0 resp. pencil
int Solver::transpose(bool forward) {
    const i64 plane = slabs[0].g.plane;
    if (!remote()) {
        for (auto &s : slabs)
            for (auto &p : slabs) {
                double *slabPtr = s.w0 + p.l0;                    // layer pitch plane
                double *penPtr = p.pencil + p.nl * s.g.t0;        // layer pitch p.nl
                if (p.nl <= 0) continue;
                if (forward)
                    DS_CHECK(xcopy2d(s, slabPtr, sizeof(double) * plane, p, penPtr, sizeof(double) * p.nl,
                                     sizeof(double) * p.nl, (size_t)s.g.ntl));
                else
                    DS_CHECK(xcopy2d(p, penPtr, sizeof(double) * p.nl, s, slabPtr, sizeof(double) * plane,
                                     sizeof(double) * p.nl, (size_t)s.g.ntl));
            }
        return 0;
    }
    // one slab per process: pack the part of every peer contiguously (one kernel), then one send/recv per peer;
    // the own part is a plain device copy
    Rccl &api = rccl_api();
    Slab &s = slabs[0];
    std::vector<i64> off(world + 1, 0), pl0(world), pnl(world), pt0(world), pntl(world);
    PencilCuts pc{};
    pc.world = world;
    for (int j = 0; j < world; ++j) {
        i64 a, b;
        pencil_range(plane, world, j, &a, &b);
        pl0[j] = a;
        pnl[j] = b - a;
        pc.cut[j] = a;
        pc.cut[j + 1] = b;
        dotsocp_slab_range_impl(nt, world, j, &a, &b);
        pt0[j] = a;
        pntl[j] = b - a;
        off[j + 1] = off[j] + pnl[j] * s.g.ntl;
    }
    auto self_copy = [&](bool fwd) -> int {
        if (s.nl <= 0) return 0;
        double *st_ = s.stage + off[rank], *pe = s.pencil + s.nl * pt0[rank];
        const size_t bytes = sizeof(double) * (size_t)(s.nl * s.g.ntl);
        DS_HIP(ds_memcpy_async(fwd ? pe : st_, fwd ? st_ : pe, bytes, hipMemcpyDeviceToDevice, stream));
        return 0;
    };
    if (forward) {
        DS_CHECK(launch_pencil_pack(true, pc, plane, s.g.ntl, s.w0, s.stage, stream));
        DS_CHECK(self_copy(true));
        DS_CHECK(comm_enter());
        const hipStream_t cs = cst(s);
        DS_NCCL(api.GroupStart());
        ++open_groups;
        for (int j = 0; j < world; ++j) {
            if (j == rank) continue;
            if (pnl[j] > 0)
                DS_NCCL_G(api.Send(s.stage + off[j], (size_t)(pnl[j] * s.g.ntl), ncclDouble, j, (ncclComm_t)nccl, cs));
            if (s.nl > 0)
                DS_NCCL_G(api.Recv(s.pencil + s.nl * pt0[j], (size_t)(s.nl * pntl[j]), ncclDouble, j, (ncclComm_t)nccl, cs));
        }
        --open_groups;
        DS_NCCL(api.GroupEnd());
        DS_CHECK(comm_leave());
    } else {
        DS_CHECK(self_copy(false));
        DS_CHECK(comm_enter());
        const hipStream_t cs = cst(s);
        DS_NCCL(api.GroupStart());
        ++open_groups;
        for (int j = 0; j < world; ++j) {
            if (j == rank) continue;
            if (s.nl > 0)
                DS_NCCL_G(api.Send(s.pencil + s.nl * pt0[j], (size_t)(s.nl * pntl[j]), ncclDouble, j, (ncclComm_t)nccl, cs));
            if (pnl[j] > 0)
                DS_NCCL_G(api.Recv(s.stage + off[j], (size_t)(pnl[j] * s.g.ntl), ncclDouble, j, (ncclComm_t)nccl, cs));
        }
        --open_groups;
        DS_NCCL(api.GroupEnd());
        DS_CHECK(comm_leave());
        DS_CHECK(launch_pencil_pack(false, pc, plane, s.g.ntl, s.w0, s.stage, stream));
    }
    return 0;
}

// --------------------------------------------------------------------------------------
// Time-slab Poisson solve without transposes (tri.hip): local eliminations, 2 numbers per mode to the mode's owner,
// reduced systems there, 2 numbers per mode back, local solves.
// --------------------------------------------------------------------------------------
static void tri_layout(i64 plane, i64 nt, int world, PencilCuts &pc, std::vector<i64> &slab_n) {
    pc.world = world;
    slab_n.assign(world, 0);
    for (int j = 0; j < world; ++j) {
        i64 a, b;
        pencil_range(plane, world, j, &a, &b);
        pc.cut[j] = a;
        pc.cut[j + 1] = b;
        dotsocp_slab_range_impl(nt, world, j, &a, &b);
        slab_n[j] = b - a;
    }
}

int Solver::tri_alloc() {
    const i64 plane = slabs[0].g.plane;
    for (auto &s : slabs) {
        if (s.tri_send) continue;
        DS_CHECK(use(s));
        DS_CHECK(s.zalloc(&s.tri_send, 2 * plane + (i64)TRI_EXTRA * world));
        DS_CHECK(s.zalloc(&s.tri_brecv, 2 * plane + (i64)TRI_EXTRA * world));
        DS_CHECK(s.zalloc(&s.tri_recv, (2 * s.nl + TRI_EXTRA) * world));
        DS_CHECK(s.zalloc(&s.tri_bsend, (2 * s.nl + TRI_EXTRA) * world));
        DS_CHECK(s.zalloc(&s.tri_zero, nt));
    }
    return 0;
}

// back == false: every slab's message for owner j -> owner j (slot of the sending slab); back == true: the way back
int Solver::tri_exchange(bool back) {
    const i64 plane = slabs[0].g.plane;
    PencilCuts pc{};
    std::vector<i64> slab_n;
    tri_layout(plane, nt, world, pc, slab_n);
    auto off = [&](int j) { return 2 * pc.cut[j] + (i64)TRI_EXTRA * j; };                  // in tri_send / tri_brecv
    auto cnt = [&](int j) { return 2 * (pc.cut[j + 1] - pc.cut[j]) + (i64)TRI_EXTRA; };  // message for / from owner j
    DS_CHECK(comm_enter());
    if (!remote()) {
        // Slabs of one process: every receiver pulls all its messages with ONE launch (peer pointers; P launches and
        // P * P stream waits instead of P * P event-ordered copies, whose host cost grew to 2.8 ms per iteration at
        // eight slabs).  "Message written" is one event per slab; the buffers need no event for their reuse: a sender
        // overwrites its message only behind its own next gather, which waits for every receiver of this one.
        const bool gather = pull_default("DOTSOCP_TRI_GATHER");
        if (gather) {
            bool one = true;
            for (auto &s : slabs) one = one && cst(s) == cst(slabs[0]);
            if (!one) {
                FOR_SLABS(s) DS_HIP(ds_event_record(s.ev[EV_TRI], cst(s)));
            }
            FOR_SLABS(sd) {                 // receiver: owner j (forward), slab p (back)
                GatherMsgs m{};
                m.n = 0;
                for (auto &ss : slabs) {    // sender
                    if (cst(ss) != cst(sd)) DS_HIP(ds_stream_wait_event(cst(sd), ss.ev[EV_TRI], 0));
                    const int d = sd.index, q = ss.index;
                    if (!back) {            // slab q's message for owner d
                        m.src[m.n] = ss.tri_send + off(d);
                        m.dst[m.n] = sd.tri_recv + (i64)q * cnt(d);
                        m.count[m.n] = cnt(d);
                    } else {                // owner q's answer for slab d
                        m.src[m.n] = ss.tri_bsend + (i64)d * cnt(q);
                        m.dst[m.n] = sd.tri_brecv + off(q);
                        m.count[m.n] = cnt(q);
                    }
                    ++m.n;
                }
                DS_CHECK(launch_gather_msgs(m, cst(sd)));
            }
            return comm_leave();
        }
        for (auto &sp : slabs)             // slab p
            for (auto &sj : slabs) {       // owner j
                const int p = sp.index, j = sj.index;
                double *a = sp.tri_send + off(j), *b = sj.tri_recv + (i64)p * cnt(j);
                if (back) { a = sj.tri_bsend + (i64)p * cnt(j); b = sp.tri_brecv + off(j); }
                if (back) DS_CHECK(xcopy(sj, a, sp, b, cnt(j)));
                else DS_CHECK(xcopy(sp, a, sj, b, cnt(j)));
            }
        return comm_leave();
    }
    // one slab per process.  The rank's own part does not travel: k_tri_reduced reads it where k_tri_local wrote it and
    // k_tri_final reads the answer where k_tri_reduced left it (launch_tri_reduced / _final: `own`)
    Rccl &api = rccl_api();
    Slab &s = slabs[0];
    const hipStream_t cs = cst(s);
    DS_NCCL(api.GroupStart());
    ++open_groups;
    for (int j = 0; j < world; ++j) {
        if (j == rank) continue;
        if (!back) {
            DS_NCCL_G(api.Send(s.tri_send + off(j), (size_t)cnt(j), ncclDouble, j, (ncclComm_t)nccl, cs));
            DS_NCCL_G(api.Recv(s.tri_recv + (i64)j * cnt(rank), (size_t)cnt(rank), ncclDouble, j, (ncclComm_t)nccl, cs));
        } else {
            DS_NCCL_G(api.Send(s.tri_bsend + (i64)j * cnt(rank), (size_t)cnt(rank), ncclDouble, j, (ncclComm_t)nccl, cs));
            DS_NCCL_G(api.Recv(s.tri_brecv + off(j), (size_t)cnt(j), ncclDouble, j, (ncclComm_t)nccl, cs));
        }
    }
    --open_groups;
    DS_NCCL(api.GroupEnd());
    return comm_leave();
}

// hooks (asynchronous schedule of step(), messages on the second streams): the latency-bound middle of the solve -- local
// eliminations, interface exchange, reduced systems, interface exchange: two small kernels and two rounds of messages --
// runs on the SECOND streams while hooks->fill (the last cone chunk) keeps the main streams busy; hooks->behind is called
// once both have been joined (more messages for the second streams).
int Solver::poisson_t_tridiag(const PhiHooks *hooks) {
    const i64 plane = slabs[0].g.plane;
    // the (0, 0) line of a slab travels whole in the TRI_EXTRA doubles behind a message (poisson_all asks before it calls)
    for (i64 p = 0, a, b; p < world; ++p) {
        dotsocp_slab_range_impl(nt, world, (int)p, &a, &b);
        if (b - a > TRI_EXTRA) {
            set_error("partitioned t-solve: slab %d has %lld time nodes, a message holds %d", (int)p, (long long)(b - a), TRI_EXTRA);
            return DOTSOCP_EINVAL;
        }
    }
    DS_CHECK(tri_alloc());
    PencilCuts pc{};
    std::vector<i64> slab_n;
    tri_layout(plane, nt, world, pc, slab_n);
    const double kscale = D * D;
    const bool async = hooks != nullptr && comm_z;
    auto own_off = [&](const Slab &s) { return 2 * pc.cut[s.index] + (i64)TRI_EXTRA * s.index; };
    if (async) {
        DS_CHECK(comm_fork());
        comm_async = true;
    }
    // (synchronous form: kernels on the main streams, every exchange forks and joins by itself)
    FOR_SLABS(s) DS_CHECK(launch_tri_local(s.g, nt, kscale, s.res->cy, s.res->cx, pc, s.w0, s.tri_send, async ? cst(s) : s.st));
    int rc = 0;
    prof_begin(PH_TRANSPOSE, async);
    rc = tri_exchange(false);
    prof_end(PH_TRANSPOSE, async);
    if (rc == 0) {
        for (auto &s : slabs) {
            if ((rc = use(s)) != 0) break;
            const bool own = remote();       // one slab per process: the own message stays where it is (tri_exchange)
            rc = launch_tri_reduced(s.g, nt, kscale, s.res->cy, s.res->cx, pc, s.index, s.l0, s.nl, slab_n.data(), s.tri_recv,
                                    s.tri_bsend, s.tri_zero, async ? cst(s) : s.st, own ? s.tri_send + own_off(s) : nullptr,
                                    own ? s.tri_brecv + own_off(s) : nullptr);
            if (rc != 0) break;
        }
    }
    if (rc == 0) {
        prof_begin(PH_TRANSPOSE, async);
        rc = tri_exchange(true);
        prof_end(PH_TRANSPOSE, async);
    }
    comm_async = false;
    DS_CHECK(rc);
    if (async) DS_CHECK(comm_mark(EV_HALO));
    if (hooks && hooks->fill) {
        prof_end(PH_POISSON);
        DS_CHECK(hooks->fill());
        prof_begin(PH_POISSON);
    }
    if (async) DS_CHECK(comm_wait(EV_HALO));
    if (hooks && hooks->behind) DS_CHECK(hooks->behind());
    FOR_SLABS(s) DS_CHECK(launch_tri_final(s.g, nt, kscale, s.res->cy, s.res->cx, pc, s.tri_brecv, s.w0, s.st));
    return 0;
}

// adjoint sums of every slab's last cell for the first edge layer of its right neighbour (kernel, main streams)
int Solver::make_tails() {
    if (!multi()) return 0;
    FOR_SLABS(s)
        if (!s.g.last) DS_CHECK(launch_tail_finalize(s.g, lc, s.fg, s.q2, s.sx, s.sy, s.send_bx, s.send_by, s.st));
    return 0;
}

int Solver::send_tails() {
    if (!multi()) return 0;
    prof_begin(PH_COMM, comm_z);
    DS_CHECK(group_begin());
    DS_CHECK(shift(+1, [](Slab &s) { return s.send_bx; }, [](Slab &s) { return s.tail_bx; }, slabs[0].g.bxLayer));
    DS_CHECK(shift(+1, [](Slab &s) { return s.send_by; }, [](Slab &s) { return s.tail_by; }, slabs[0].g.byLayer));
    DS_CHECK(group_end());
    prof_end(PH_COMM, comm_z);
    return 0;
}

// first phi layer of every slab -> halo layer of its left neighbour (forward time difference of the q-step)
int Solver::send_phi_head() {
    if (!multi()) return 0;
    prof_begin(PH_COMM, comm_z);
    DS_CHECK(shift(-1, [](Slab &s) { return s.phi; }, [](Slab &s) { return s.phi + s.g.plane * s.g.ntl; }, slabs[0].g.plane));
    prof_end(PH_COMM, comm_z);
    return 0;
}

int Solver::ship_tails() {
    if (multi()) {
        DS_CHECK(make_tails());
        DS_CHECK(group_begin());        // one group: traffic in both directions at once
        DS_CHECK(send_phi_head());
        DS_CHECK(send_tails());
        DS_CHECK(group_end());
    }
    return 0;
}

}  // namespace dotsocp
