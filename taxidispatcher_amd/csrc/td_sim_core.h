// td_sim_core.h — the per-element rules of the device-resident simulator worlds (td_sim.hip, td_simb.hip), one place each.
// The kernels that apply them, and the host helpers of both handles, are in td_sim_world.h.
//
// Every rule is a statement-by-statement port of taxidispatcher_amd/simulator.py (the harness with Simulator.java's
// semantics; SURVEY.md Appendix A lists the bug-compatible details).  Requests are addressed by their INDEX in the
// request table everywhere on the device (the reference looks ids up in a dictionary; ids are unique, so the index is
// the same thing); ids appear again only where the reference stores one (pool_id, and the client reported by td_sim_state).
#pragma once
#include <stdint.h>

#include "taxidispatcher_amd.h"

namespace tdsim {

constexpr int CB = 1024;                 // workgroup of every compaction pass: 16 waves, one element per thread
constexpr int32_t NONE = 0x7f7f7f7f;     // "no pair / no plan" (what a byte-wise fill with 0x7f leaves)

// the world in HBM; passed to the kernels by value
struct World {
    int n_cabs, n_req, n_stands, drop_time, big_cost;
    // request table
    const int32_t *r_id, *r_from, *r_to, *r_at;
    int32_t *r_cab, *r_pick, *r_pid, *r_plan, *r_pcost;
    // fleet (c_clnt = request INDEX, -1 = none)
    int32_t *c_from, *c_to, *c_clnt, *c_onb, *c_start;
    // the city: a stand-to-stand table [from][to] of n_stands x n_stands entries, nullptr = the line (|a - b|)
    const int32_t *dist;
};

// device counters of one world: the sums of Simulator.m (64-bit), an error word (td_sim's; a batch has one for the handle)
// and this tick's OPT count.  The list sizes are offset arrays of the handles.
struct Ctl {
    long long dropped, pickup_time, pickup_numb, second;
    int32_t err;        // 1: internal, 2: a pair or plan index handed in lies outside its list, 3: an invalid distance table
    int32_t opt_count, pad[6];
};
static_assert(sizeof(Ctl) == 64, "both handles lay a Ctl out as 16 ints");

// ---- the event log (td_sim_log / td_simb_log).  Every record a rule can write has a fixed slot in a staging
// array of its phase; a slot is four words {kind | method << 8, customer id, cab number, aux}, kind 0 = no record.  The rules
// take an emitter: EvOff is empty and compiles to nothing (the instantiation every handle uses until *_log switches logging
// on), EvOn writes the slot with one 16-byte vector store.
constexpr int EV_LCM = 1, EV_OPT = 2;   // the record's method word (0: the kind has none)
struct EvOff {
    static constexpr bool on = false;
    __device__ __forceinline__ void put(int, int, int, int, int, int) const {}
};
struct EvOn {
    static constexpr bool on = true;
    int4 *st;
    __device__ __forceinline__ void put(int slot, int kind, int method, int customer, int cab, int aux) const
    {
        st[slot] = make_int4(kind | method << 8, customer, cab, aux);
    }
};

// ---- the route model (td_sim_route).  A routed cab drives its pool's plan: 8 stop words per cab, a stop word
// = request index * 2 + (1: drop-off, 0: pick-up), -1 = no stop, and the position of the next stop to serve.  The rules take
// the route as a template parameter the way they take the event log's emitter: RouteOff is empty and compiles to nothing (the
// instantiation of every handle that never asked for routes), RouteOn holds a td_sim handle's route storage, RouteOnB a batch's.
// What a batch adds is per world, so a kernel binds the route to its world once, `rt.of(b)`, and the rules below see one
// world's route: RouteOff and RouteOn return themselves, RouteOnB a RouteOn of world b (td_simb_route).
struct RouteOff {
    static constexpr bool on = false;
    struct Acc {};
    __device__ __forceinline__ const RouteOff &of(int) const { return *this; }
};
struct RouteAcc {   // what one thread's served drop-offs add to the route counters
    long long drops = 0, ride = 0, solo = 0, over = INT64_MIN;
};
struct RouteOn {
    static constexpr bool on = true;
    using Acc = RouteAcc;
    int32_t *stops, *pos, *r_drop;   // [8 n_cabs], [n_cabs], [n_req]
    long long *cnt;                  // drop_numb, ride_time, solo_time, max_over_loss
    int loss;                        // the policy's max_loss_pct
    // what a dispatching thread builds a stop list from: the tick's 9-int records, the tick's demand list (a record's members
    // are positions in it), and the record of each customer of the demand after pooling / of the kept demand (-1: none)
    const int32_t *recs, *dem_idx, *d_rec, *kd_rec;
    __device__ __forceinline__ const RouteOn &of(int) const { return *this; }
};
// B worlds behind one handle.  Stops, positions, r_drop and the record columns are indexed by the concatenated cab / request /
// list row, as c_from and r_pick are; per world: four counters, the loss of the world's policy, its slab of `stride` records,
// and its demand list (a record's members are positions in it; what lies there indexes the concatenated request table).
struct RouteOnB {
    static constexpr bool on = true;
    using Acc = RouteAcc;
    int32_t *stops, *pos, *r_drop;
    long long *cnt;                  // [4 B]
    const int32_t *loss;             // [B]
    const int32_t *recs, *dem_idx, *d_rec, *kd_rec, *dem_off;
    int stride;
    __device__ __forceinline__ RouteOn of(int b) const
    {
        return RouteOn{stops, pos, r_drop, cnt + 4 * (size_t)b, loss[b], recs + (size_t)9 * ((size_t)b * (size_t)stride), dem_idx + dem_off[b], d_rec, kd_rec};
    }
};

// Simulator.java:469-474
__host__ __device__ inline int cheat_a_bit(int frm, int cost, int n_stands)
{
    if (frm + cost >= n_stands) return frm - cost < 0 ? 0 : frm - cost;
    return frm + cost;
}

__host__ __device__ inline int iabs(int v) { return v < 0 ? -v : v; }

// the way from stand a to stand b (the row is always the stand the cab is at or heads to)
__device__ __forceinline__ int way(const World &w, int a, int b) { return w.dist ? w.dist[(int64_t)a * w.n_stands + b] : iabs(a - b); }

// Simulator._near on the line: any flagged stand within distance < drop_time of s (bits = one bit per stand)
__device__ inline bool near_window(const uint32_t *bits, int n_stands, int drop_time, int s)
{
    const int r = (drop_time - 1 < n_stands ? drop_time - 1 : n_stands);   // a wider window sees no more stands
    const int lo = s - r < 0 ? 0 : s - r, hi = s + r > n_stands - 1 ? n_stands - 1 : s + r;
    if (lo > hi) return false;
    for (int w = lo >> 5; w <= hi >> 5; w++) {   // at most (2 r + 1) / 32 + 2 words
        uint32_t m = 0xffffffffu;
        if (w == lo >> 5) m &= 0xffffffffu << (lo & 31);
        if (w == hi >> 5) m &= 0xffffffffu >> (31 - (hi & 31));
        if (bits[w] & m) return true;
    }
    return false;
}

__device__ __forceinline__ bool bit_of(const uint32_t *bits, int s) { return (bits[s >> 5] >> (s & 31)) & 1u; }

// ---- a world on a distance table (td_sim_create_dist, td_simb_create_dist)
constexpr int32_t MAX_DIST = 0x1fffffff;   // three entries stay below td_pool2's INT_MAX diagonal marker
constexpr int MAX_DIST_STANDS = 4096;

// the neighbour bit matrices of a distance table, one thread per (stand s, word q); the row read visits every cell of the
// table exactly once, so the table is validated here: diagonal 0, every other entry in 1 .. MAX_DIST (error word 3).
// static: td_sim.hip and td_simb.hip each hold their own instance of this one definition
static __global__ __launch_bounds__(256) void k_nb_build(int n_stands, int words, int drop_time, const int32_t *__restrict__ dist,
                                                         uint32_t *__restrict__ nb_dem, uint32_t *__restrict__ nb_sup, int32_t *err)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // n_stands * words <= 4096 * 128
    if (i >= n_stands * words) return;
    const int s = i / words, q = i - s * words;
    uint32_t md = 0, ms = 0;
    bool bad = false;
    for (int b = 0; b < 32; b++) {
        const int o = q * 32 + b;
        if (o >= n_stands) break;
        const int32_t out = dist[(int64_t)s * n_stands + o], in = dist[(int64_t)o * n_stands + s];
        bad |= o == s ? out != 0 : (out < 1 || out > MAX_DIST);
        if (out < drop_time) ms |= 1u << b;
        if (in < drop_time) md |= 1u << b;
    }
    nb_dem[i] = md;
    nb_sup[i] = ms;
    if (bad) atomicMax(err, 3);
}

// Simulator._advance: cab c has just reached stand `cur` at tick t with the stop words s[8] and `pos` stops served.  Every stop
// at this stand is served now (a zero-length leg); then the cab starts for the next stop's stand, or, with none left, is free
// here in this tick.  The loop is unrolled over the eight words, which stay in registers; `go` ends it at the first stop elsewhere.
__device__ __forceinline__ void route_advance(const World &w, const RouteOn &rt, int t, int c, int cur, const int (&s)[8], int pos, RouteAcc &acc)
{
    bool go = true;
    int next = -1;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (go && i >= pos) {
            const int wd = s[i];
            if (wd < 0) {
                go = false;
            } else {
                const int req = wd >> 1, drop = wd & 1;
                const int st = drop ? w.r_to[req] : w.r_from[req];
                if (st != cur) {
                    next = st;
                    go = false;
                } else if (drop) {
                    const long long ride = t - w.r_pick[req], solo = way(w, w.r_from[req], st);
                    const long long over = ride * 100 - solo * (100 + rt.loss);
                    rt.r_drop[req] = t;
                    acc.drops++;
                    acc.ride += ride;
                    acc.solo += solo;
                    acc.over = over > acc.over ? over : acc.over;
                    pos = i + 1;
                } else {
                    w.r_pick[req] = t;
                    pos = i + 1;
                }
            }
        }
    }
    rt.pos[c] = pos;
    w.c_from[c] = cur;
    if (next >= 0) {
        w.c_to[c] = next;
        w.c_onb[c] = 1;
        w.c_start[c] = t;
    } else {   // today's "cab is free" state
        w.c_to[c] = cur;
        w.c_clnt[c] = -1;
        w.c_onb[c] = 0;
        w.c_start[c] = -1;
    }
}

// the stop words of record `rec` into s and into the cab's list (two 16-byte stores): the path pn_check prices, the pick-ups in
// order, then the drop-offs in order (k of each in the record, -1 behind them; members are positions in the tick's demand list)
__device__ __forceinline__ void route_give(const RouteOn &rt, int cab, int rec, int (&s)[8])
{
    const int32_t *r = rt.recs + (size_t)9 * rec;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) k += r[i] >= 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = i < k ? 2 * rt.dem_idx[r[i]] : i < 2 * k ? 2 * rt.dem_idx[r[4 + i - k]] + 1 : -1;
    ((int4 *)rt.stops)[2 * (size_t)cab] = make_int4(s[0], s[1], s[2], s[3]);
    ((int4 *)rt.stops)[2 * (size_t)cab + 1] = make_int4(s[4], s[5], s[6], s[7]);
}

// the cab's stop words in registers (two 16-byte loads); true when a stop is left at its position
__device__ __forceinline__ bool route_load(const RouteOn &rt, int c, int (&s)[8], int *pos)
{
    const int4 a = ((const int4 *)rt.stops)[2 * (size_t)c], b = ((const int4 *)rt.stops)[2 * (size_t)c + 1];
    s[0] = a.x, s[1] = a.y, s[2] = a.z, s[3] = a.w, s[4] = b.x, s[5] = b.y, s[6] = b.z, s[7] = b.w;
    const int p = rt.pos[c];
    *pos = p;
    int at = -1;
#pragma unroll
    for (int i = 0; i < 8; i++) at = i == p ? s[i] : at;
    return at >= 0;
}

// Simulator.java:220-254 for ONE cab; returns 1 when a passenger was picked up.  c = the cab's row in the fleet table,
// cab_no = the number the request table stores for it (the same thing in one world; world-local in a batch of worlds).
// The cab's record (:233 picked up, :251 free, or none) goes to `slot` of ev: every cab writes its slot in every tick.
// rt: RouteOff, or RouteOn: a cab with stops left serves the stop it has reached and advances (acc: its drop-offs' counters)
template <class EV, class R>
__device__ inline int arrive_as(const World &w, int t, int c, int cab_no, const EV &ev, int slot, const R &rt, typename R::Acc &acc)
{
    static_assert(!(EV::on && R::on), "the event log of routed worlds is not built");
    const int f = w.c_from[c], to = w.c_to[c];
    ev.put(slot, 0, 0, -1, -1, -1);
    if (f == to || way(w, f, to) != t - w.c_start[c]) return 0;
    if (w.c_onb[c] == 0) {
        const int d = w.c_clnt[c];
        if (d < 0) return 0;
        if constexpr (EV::on) ev.put(slot, TD_EV_PICKED_UP, 0, w.r_id[d], cab_no, -1);
        w.r_cab[d] = cab_no;
        if constexpr (R::on) {
            int s[8], pos;
            if (route_load(rt, c, s, &pos)) {   // the arrival serves stop 0 and advances; the pool info of the table is not looked at
                route_advance(w, rt, t, c, to, s, pos, acc);
                return 1;
            }
        }
        w.r_pick[d] = t;
        w.c_from[c] = w.r_from[d];
        w.c_to[c] = w.r_pid[d] == -1 ? w.r_to[d] : cheat_a_bit(w.r_from[d], w.r_pcost[d], w.n_stands);
        w.c_onb[c] = 1;
        w.c_start[c] = t;
        return 1;
    }
    if constexpr (R::on) {
        int s[8], pos;
        if (route_load(rt, c, s, &pos)) {
            route_advance(w, rt, t, c, to, s, pos, acc);
            return 0;
        }
    }
    w.c_from[c] = to;
    w.c_clnt[c] = -1;
    w.c_onb[c] = 0;
    w.c_start[c] = -1;
    ev.put(slot, TD_EV_CAB_FREE, 0, -1, cab_no, to);
    return 0;
}

// Simulator.java:424-490 _dispatch for cab `cab` (standing at sup_to) and the customer (request idx, pool partner / cost).
// The record (:448-465 or :486-487, with `method`) goes to `slot` of ev; cab_no is the cab's number as the log prints it.
// rt / rec / acc: RouteOff, or RouteOn and the customer's record (-1: none, the customer behaves as without routes): the cab
// receives the record's stop list; standing at the first pick-up it serves stop 0 now and advances, cheat_a_bit is not called
template <class EV, class R>
__device__ __forceinline__ void dispatch(const World &w, int t, int cab, int sup_to, int idx, int partner, int pcost, int &numb, int &ptime,
                                         const EV &ev, int slot, int method, int cab_no, const R &rt, int rec, typename R::Acc &acc)
{
    const int cf = w.r_from[idx];
    int dn = 0, dp = 0;   // added to the counters once, below: no store through either reference inside a branch
    bool routed = false;
    if constexpr (R::on) routed = rec >= 0;
    if (sup_to == cf) {   // assignToCabAndGo
        if (routed) {
            if constexpr (R::on) {
                int s[8];
                route_give(rt, cab, rec, s);
                w.c_clnt[cab] = idx;
                route_advance(w, rt, t, cab, cf, s, 0, acc);
            }
        } else {
            w.c_from[cab] = cf;
            w.c_to[cab] = partner == -1 ? w.r_to[idx] : cheat_a_bit(cf, pcost, w.n_stands);
            w.c_clnt[cab] = idx;
            w.c_onb[cab] = 1;
            w.c_start[cab] = t;
        }
        dn = 1;
        if constexpr (EV::on) ev.put(slot, TD_EV_ASSIGNED_PICKED, method, w.r_id[idx], cab_no, partner == -1 ? -1 : w.r_id[partner]);
    } else if (way(w, sup_to, cf) < w.drop_time) {   // goToPickup
        w.c_to[cab] = cf;
        w.c_clnt[cab] = idx;
        w.c_onb[cab] = 0;
        w.c_start[cab] = t;
        dp = way(w, w.c_from[cab], cf);
        if constexpr (R::on) {
            if (routed) {   // the arrival serves stop 0
                int s[8];
                route_give(rt, cab, rec, s);
                rt.pos[cab] = 0;
            }
        }
        if constexpr (EV::on) ev.put(slot, TD_EV_HEADING, method, w.r_id[idx], cab_no, -1);
    }
    numb += dn;
    ptime += dp;
}

}  // namespace tdsim
