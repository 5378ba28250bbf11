// continuum_plan.cpp -- see continuum_plan.h.  Pure host code (no HIP include).
#include "continuum_plan.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <tuple>

#include "../../include/dftatom_hip.h"

namespace dfta_continuum_plan {

static_assert(kMaxPartners == DFTA_CONT_MAX_PARTNERS, "continuum_plan.h and the header disagree");
static_assert(kLmax == DFTA_BESSEL_LMAX, "continuum_plan.h and the header disagree");

const char* check(const Call& c)
{
    if (c.norm_mode != DFTA_CONT_FREE && c.norm_mode != DFTA_CONT_WKB) return "continuum: norm_mode (DFTA_CONT_FREE or DFTA_CONT_WKB)";
    if (c.N < 5) return "continuum: the grid needs 5 nodes";
    if (c.nV < 1) return "continuum: nV";
    if (c.power < 0 || c.power > kMaxPower) return "continuum: power outside 0 .. 8";
    if (c.npartner_rows < 0 || c.nlists < 0) return "continuum: npartner_rows, nlists";
    if (c.nlists > 0) {
        if (!c.list_off || c.list_off[0] != 0) return "continuum: list_off must start at 0";
        for (int k = 0; k < c.nlists; ++k) {
            const int n = c.list_off[k + 1] - c.list_off[k];
            if (n < 0) return "continuum: list_off must ascend";
            if (n > kMaxPartners) return "continuum: more than 16 partners in a list";
        }
        if (c.list_off[c.nlists] > 0 && !c.list_rows) return "continuum: list_rows";
        for (int j = 0; j < c.list_off[c.nlists]; ++j)
            if (c.list_rows[j] < 0 || c.list_rows[j] >= c.npartner_rows) return "continuum: a partner row outside 0 .. npartner_rows-1";
    }
    for (int t = 0; t < c.ntrials; ++t) {
        if (c.vidx && (c.vidx[t] < 0 || c.vidx[t] >= c.nV)) return "continuum: a potential index outside 0 .. nV-1";
        if (c.l[t] < 0 || c.l[t] > kLmax) return "continuum: l outside 0 .. 4";
        if (!std::isfinite(c.E[t])) return "continuum: E must be finite";
        if (c.m[t] < 3 || c.m[t] > c.N - 2) return "continuum: m outside 3 .. N-2";
        if (c.trial_list && (c.trial_list[t] < -1 || c.trial_list[t] >= c.nlists)) return "continuum: a trial's list outside -1 .. nlists-1";
    }
    return nullptr;
}

int instance_for(int n) { return n <= 0 ? 0 : (n <= 4 ? 4 : (n <= 8 ? 8 : 16)); }

Plan plan(const Call& c, bool want_rows)
{
    Plan p;
    typedef std::tuple<int, int, int> Key;
    std::map<Key, int> index;                        // group -> its number, in the order of first appearance
    std::vector<Key> keys;
    std::vector<std::vector<int>> members;
    for (int t = 0; t < c.ntrials; ++t) {
        const Key k(c.vidx ? c.vidx[t] : 0, c.l[t], c.trial_list ? c.trial_list[t] : -1);
        auto it = index.find(k);
        if (it == index.end()) {
            it = index.emplace(k, (int)keys.size()).first;
            keys.push_back(k);
            members.emplace_back();
        }
        members[it->second].push_back(t);
    }
    int longest = 0;
    for (size_t gi = 0; gi < keys.size(); ++gi) {
        const int list = std::get<2>(keys[gi]);
        if (list >= 0) longest = std::max(longest, c.list_off[list + 1] - c.list_off[list]);
        const std::vector<int>& mem = members[gi];
        for (size_t at = 0; at < mem.size(); at += kWave) {
            Block b;
            b.v = std::get<0>(keys[gi]); b.l = std::get<1>(keys[gi]); b.list = list;
            b.first = (int)p.order.size();
            b.cnt = (int)std::min<size_t>(kWave, mem.size() - at);
            for (int j = 0; j < kWave; ++j) p.order.push_back(j < b.cnt ? mem[at + j] : -1);
            p.blocks.push_back(b);
        }
    }
    p.instance = instance_for(longest);
    if (want_rows) {
        const size_t per_block = sizeof(double) * kWave * (size_t)c.N;
        const size_t fit = std::min<size_t>(kRowBudgetBytes / per_block, kMaxChunkBlocks);
        p.blocks_per_chunk = (int)std::max<size_t>(1, std::min<size_t>(fit, p.blocks.size()));
    }
    return p;
}

}  // namespace dfta_continuum_plan
