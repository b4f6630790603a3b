// td_sim_layout.h — where the arrays of a world handle lie: the device block and the pinned block of td_sim (one world)
// and td_simb (B worlds), each written once as a function of a td::Carve.  Run on a null base a layout gives the block's
// size, run on the allocation it sets the pointers; no sum has to agree with it.  Host code without HIP: the handles
// inherit the pointer structs, tests/stage_host_main.cpp checks the layouts.
#pragma once
#include "td_stage.h"

namespace tdsim {

// the world tables both handles keep (World of td_sim_core.h points at them)
struct WorldDev {
    int32_t *r_id, *r_from, *r_to, *r_at, *r_cab, *r_pick, *r_pid, *r_plan, *r_pcost;
    int32_t *c_from, *c_to, *c_clnt, *c_onb, *c_start;
};

// and the per-tick lists of both: nr requests, nc cabs in all
struct ListsDev : WorldDev {
    // temp lists: demand before pooling, supply, demand after pooling, kept lists
    int32_t *dem_idx, *dem_from, *dem_to;
    int32_t *sup_cab, *sup_to;
    int32_t *d2_idx, *d2_from, *d2_partner, *d2_plan, *d2_cost;
    int32_t *ks_cab, *ks_to;
    int32_t *kd_idx, *kd_from, *kd_partner, *kd_plan, *kd_cost;
    int32_t *isb, *ainfo;          // analyzePool: is a B customer / first plan as the A customer
    int32_t *pair_cab, *pair_dem;  // first pair of a cab / request
};

// the order in which both handles have always laid them out; what only one handle has goes in where it always lay: behind
// the demand (nr each), behind the pooled demand (nr each), and the plan lists (n_plans each) in front of the pair maps
using Lists = std::initializer_list<int32_t **>;
inline void lists_layout(td::Carve &c, size_t nr, size_t nc, ListsDev &l, Lists after_dem, Lists after_d2, Lists plans, size_t n_plans)
{
    for (int32_t **a : {&l.r_id, &l.r_from, &l.r_to, &l.r_at, &l.r_cab, &l.r_pick, &l.r_pid, &l.r_plan, &l.r_pcost}) *a = c.take<int32_t>(nr);
    for (int32_t **a : {&l.c_from, &l.c_to, &l.c_clnt, &l.c_onb, &l.c_start}) *a = c.take<int32_t>(nc);
    for (int32_t **a : {&l.dem_idx, &l.dem_from, &l.dem_to}) *a = c.take<int32_t>(nr);
    for (int32_t **a : after_dem) *a = c.take<int32_t>(nr);
    for (int32_t **a : {&l.sup_cab, &l.sup_to}) *a = c.take<int32_t>(nc);
    for (int32_t **a : {&l.d2_idx, &l.d2_from, &l.d2_partner, &l.d2_plan, &l.d2_cost}) *a = c.take<int32_t>(nr);
    for (int32_t **a : after_d2) *a = c.take<int32_t>(nr);
    for (int32_t **a : {&l.ks_cab, &l.ks_to}) *a = c.take<int32_t>(nc);
    for (int32_t **a : {&l.kd_idx, &l.kd_from, &l.kd_partner, &l.kd_plan, &l.kd_cost, &l.isb, &l.ainfo}) *a = c.take<int32_t>(nr);
    for (int32_t **a : plans) *a = c.take<int32_t>(n_plans);
    l.pair_cab = c.take<int32_t>(nc);
    l.pair_dem = c.take<int32_t>(nr);
}

// ---- td_sim ----------------------------------------------------------------------------------------------------------
constexpr size_t SIM_HEAD_INTS = 64;   // ints reserved for the head block
constexpr size_t SIM_PIN_HEAD = 256;   // bytes of the pinned block in front of td_tick's host results

struct SimDims {
    size_t nc, nr;       // cabs; requests, at least 1
    size_t cap;          // of every per-tick list: max(nc, nr)
    size_t words;        // of one stand bitset
    size_t blocks;       // compaction workgroups over cap elements
    size_t ns;           // stands
    bool dist;           // a table world
};

struct SimDev : ListsDev {
    int32_t *head_blk = nullptr;   // Ctl and the per-tick list sizes
    uint32_t *bits = nullptr;      // cab bits, then request bits: the batched layout at b == 0
    // a table world: the table, the neighbour bit matrices [n_stands][words], the near bitsets (laid out like bits)
    int32_t *dist = nullptr;
    uint32_t *nb_dem = nullptr, *nb_sup = nullptr, *near = nullptr;
    int32_t *blockcnt = nullptr;
    int32_t *pl_a, *pl_b, *pl_plan, *pl_cost;   // td_pool2's plan list
    int32_t *in_rows, *in_cols, *in_r2c;        // this tick's decisions
    int32_t *tmp;                               // td_sim_state: client ids
};

inline void sim_layout(td::Carve &c, const SimDims &d, SimDev &s)
{
    s.head_blk = c.take<int32_t>(SIM_HEAD_INTS);
    // the cab bits and the request bits must stay adjacent, in this order (and so the two near bitsets): the kernels address
    // them as world 0 of the batched layout, and sim_begin clears both with ONE memset
    s.bits = c.take<uint32_t>(2 * d.words);
    if (d.dist) {
        s.near = c.take<uint32_t>(2 * d.words);
        s.nb_dem = c.take<uint32_t>(d.ns * d.words);
        s.nb_sup = c.take<uint32_t>(d.ns * d.words);
        s.dist = c.take<int32_t>(d.ns * d.ns);
    }
    s.blockcnt = c.take<int32_t>(d.blocks);
    lists_layout(c, d.nr, d.nc, s, {}, {}, {&s.pl_a, &s.pl_b, &s.pl_plan, &s.pl_cost}, d.nr / 2 + 1);
    for (int32_t **a : {&s.in_rows, &s.in_cols, &s.in_r2c, &s.tmp}) *a = c.take<int32_t>(d.cap);
}

// pinned: the head's read-back, then td_tick's host results for td_sim_step
struct SimPin {
    char *h_head = nullptr;
    int32_t *h_rows, *h_cols, *h_kc, *h_kd, *h_r2c;
};

inline void sim_pin_layout(td::Carve &c, const SimDims &d, SimPin &p)
{
    p.h_head = c.take<char>(SIM_PIN_HEAD);
    for (int32_t **a : {&p.h_rows, &p.h_cols, &p.h_kc, &p.h_kd, &p.h_r2c}) *a = c.take<int32_t>(d.cap);
}

// ---- td_simb ---------------------------------------------------------------------------------------------------------
constexpr size_t SIMB_N_OFF = 7;   // offset arrays of the head block
constexpr size_t SIMB_N_PER = 4;   // per-world words of the head block

struct SimbDims {
    size_t nb, nc, nr;       // worlds; cabs of all worlds; requests of all worlds, at least 1
    size_t words, ns;        // of one stand bitset; stands
    size_t n_cnt;            // per-workgroup counts of one compaction pass over all worlds
    size_t pool_cap, in_cap, tk_cap;   // plans; decisions handed in; td_tick_batched's strided outputs
    size_t tmp;              // the largest fleet, at least 1
    bool dist;               // a table batch
    // Ctl[B], the error word (16 ints), the offset arrays, the per-world words: what one copy brings to the host
    size_t head_ints() const { return 16 * nb + 16 + SIMB_N_OFF * (nb + 1) + SIMB_N_PER * nb; }
    // of the pinned stage: the offsets and flags of td_simb_apply, or the initial tables
    size_t stage_ints() const { return std::max<size_t>(3 * (nb + 1), 2 * (nb + 1) + 5 * nc + 5 * nr); }
};

struct SimbDev : ListsDev {
    int64_t *p_total, *tk_total;
    // head block: Ctl[B] (ctl_blk), the error word, the offset arrays, the per-world words
    int64_t *ctl_blk = nullptr;
    int32_t *gerr = nullptr;
    int32_t *dem_off, *sup_off, *pl_off, *d2_off, *tk_off, *ks_off, *kd_off;
    int32_t *n_pools, *tk_np, *tk_lm, *tk_rest;
    int32_t *d_cab_off = nullptr, *d_req_off = nullptr;
    uint32_t *bits = nullptr;    // world b: cab bits at (2 b) * words, request bits at (2 b + 1) * words
    // a table batch: the table, the neighbour bit matrices [n_stands][words] and the near bitsets, laid out like bits
    int32_t *dist = nullptr;
    uint32_t *nb_dem = nullptr, *nb_sup = nullptr, *near = nullptr;
    int32_t *cnt_a, *cnt_b;
    int32_t *pl_from, *pl_to, *tk_from;         // the pooled demand, the demand td_tick_batched is handed
    int32_t *pa, *pb, *pp, *pc;                 // the pool calls' plan lists
    int32_t *in_rows, *in_cols, *in_r2c, *in_pair_off, *in_r2c_off, *in_solved;
    int32_t *tk_rows, *tk_cols, *tk_r2c;        // td_tick_batched's strided outputs
    int32_t *tmp;
    int32_t *d_none = nullptr;   // [B]: 1 = the world is left out of the pool lists
    int32_t *d_rule = nullptr;   // [B]: the world's LCM rule under td_simb_dispatch
};

inline void simb_layout(td::Carve &c, const SimbDims &d, SimbDev &s)
{
    const size_t nb = d.nb, nr = d.nr, nc = d.nc;
    // the two 64-bit arrays and the head block lie at the front, in this order: create zeroes them with one memset
    s.p_total = c.take<int64_t>(nb);
    s.tk_total = c.take<int64_t>(nb);
    s.ctl_blk = c.take<int64_t>(8 * nb);   // Ctl holds 64-bit sums
    s.gerr = c.take<int32_t>(16);
    // the seven offset arrays and the four per-world arrays are one block (zeroed per tick)
    for (int32_t **a : {&s.dem_off, &s.sup_off, &s.pl_off, &s.d2_off, &s.tk_off, &s.ks_off, &s.kd_off}) *a = c.take<int32_t>(nb + 1);
    for (int32_t **a : {&s.n_pools, &s.tk_np, &s.tk_lm, &s.tk_rest}) *a = c.take<int32_t>(nb);
    s.d_cab_off = c.take<int32_t>(nb + 1);
    s.d_req_off = c.take<int32_t>(nb + 1);
    s.bits = c.take<uint32_t>(2 * d.words * nb);
    s.cnt_a = c.take<int32_t>(d.n_cnt);
    s.cnt_b = c.take<int32_t>(d.n_cnt);
    if (d.dist) {   // one city for the whole batch
        s.near = c.take<uint32_t>(2 * d.words * nb);
        s.nb_dem = c.take<uint32_t>(d.ns * d.words);
        s.nb_sup = c.take<uint32_t>(d.ns * d.words);
        s.dist = c.take<int32_t>(d.ns * d.ns);
    }
    lists_layout(c, nr, nc, s, {&s.pl_from, &s.pl_to}, {&s.tk_from}, {&s.pa, &s.pb, &s.pp, &s.pc}, d.pool_cap);
    for (int32_t **a : {&s.in_rows, &s.in_cols, &s.in_r2c}) *a = c.take<int32_t>(d.in_cap);
    // in_pair_off, in_r2c_off and in_solved are uploaded by one copy
    s.in_pair_off = c.take<int32_t>(nb + 1);
    s.in_r2c_off = c.take<int32_t>(nb + 1);
    s.in_solved = c.take<int32_t>(nb);
    for (int32_t **a : {&s.tk_rows, &s.tk_cols, &s.tk_r2c}) *a = c.take<int32_t>(d.tk_cap);
    s.tmp = c.take<int32_t>(d.tmp);
    s.d_none = c.take<int32_t>(nb);
    s.d_rule = c.take<int32_t>(nb);
}

// pinned: the head's mirror, then a stage for the offsets / flags of td_simb_apply and the initial tables
struct SimbPin {
    int32_t *h_head = nullptr, *h_stage = nullptr;
};

inline void simb_pin_layout(td::Carve &c, const SimbDims &d, SimbPin &p)
{
    p.h_head = c.take<int32_t>(d.head_ints());
    p.h_stage = c.take<int32_t>(d.stage_ints());
}

}  // namespace tdsim
