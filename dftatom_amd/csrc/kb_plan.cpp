// kb_plan.cpp -- see kb_plan.h.  Pure host code (no HIP include).
#include "kb_plan.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <map>

#include "../../include/dftatom_hip.h"

namespace dfta_kb_plan {

static_assert(kMaxStates == DFTA_KB_MAX_STATES, "kb_plan.h and the header disagree");
static_assert(kLmax == DFTA_BESSEL_LMAX, "kb_plan.h and the header disagree");

std::vector<int> last_nonzero(int nch, int N, const double* beta)
{
    std::vector<int> out((size_t)std::max(nch, 0), 0);
    for (int k = 0; k < nch; ++k) {
        const double* row = beta + (size_t)k * N;
        int i = N - 1;
        while (i > 0 && row[i] == 0.) --i;
        out[k] = i;
    }
    return out;
}

const char* check(const Call& c, const std::vector<int>& lastnz)
{
    if (c.N < 5) return "kb: the grid needs 5 nodes";
    if (c.nV < 1 || c.nch < 1) return "kb: nV, nch";
    for (int k = 0; k < c.nch; ++k) {
        if (c.vidx && (c.vidx[k] < 0 || c.vidx[k] >= c.nV)) return "kb: a potential index outside 0 .. nV-1";
        if (c.l[k] < 0 || c.l[k] > kLmax) return "kb: l outside 0 .. 4";
        if (!std::isfinite(c.q1[k]) || c.q1[k] == 0.) return "kb: q1 must be finite and not 0";
    }
    for (int t = 0; t < c.ntrials; ++t) {
        const int k = c.chan ? c.chan[t] : 0;
        if (k < 0 || k >= c.nch) return "kb: a channel outside 0 .. nch-1";
        if (!std::isfinite(c.E[t])) return "kb: E must be finite";
        if (c.m[t] < 3 || c.m[t] > c.N - 2) return "kb: m outside 3 .. N-2";
        if (c.m[t] < lastnz[k]) return "kb: m below the last non-zero node of the projector";
    }
    return nullptr;
}

Plan plan(const Call& c, bool want_rows, int force_chunk)
{
    Plan p;
    std::map<int, int> index;                        // channel -> its group, in the order of first appearance
    std::vector<int> keys;
    std::vector<std::vector<int>> members;
    for (int t = 0; t < c.ntrials; ++t) {
        const int k = c.chan ? c.chan[t] : 0;
        auto it = index.find(k);
        if (it == index.end()) {
            it = index.emplace(k, (int)keys.size()).first;
            keys.push_back(k);
            members.emplace_back();
        }
        members[it->second].push_back(t);
    }
    for (size_t gi = 0; gi < keys.size(); ++gi) {
        const std::vector<int>& mem = members[gi];
        for (size_t at = 0; at < mem.size(); at += kWave) {
            Block b;
            b.chan = keys[gi];
            b.first = (int)p.order.size();
            b.cnt = (int)std::min<size_t>(kWave, mem.size() - at);
            for (int j = 0; j < kWave; ++j) p.order.push_back(j < b.cnt ? mem[at + j] : -1);
            p.blocks.push_back(b);
        }
    }
    if (want_rows) {
        const size_t per_block = 2 * sizeof(double) * kWave * (size_t)c.N;
        size_t fit = std::min<size_t>(kRowBudgetBytes / per_block, kMaxChunkBlocks);
        if (force_chunk > 0) fit = std::min<size_t>(fit, (size_t)force_chunk);
        p.blocks_per_chunk = (int)std::max<size_t>(1, std::min<size_t>(fit, p.blocks.size()));
    }
    return p;
}

double scan_energy(double lo, double hi, int nscan, int k) { return lo + ((hi - lo) * (double)k) / (double)(nscan - 1); }

double cut_energy(double a, double b, int j)
{
    double e = a + ((b - a) * (double)(j + 1)) / 65.;
    if (e < a) e = a;
    if (e > b) e = b;
    return e;
}

bool bracket_closed(double a, double b) { return std::nextafter(a, std::numeric_limits<double>::infinity()) >= b; }

std::vector<Bracket> open_brackets(int nscan, const double* E, const unsigned char* finite, const unsigned char* neg)
{
    std::vector<Bracket> out;
    for (int k = 0; k + 1 < nscan && (int)out.size() < kMaxStates; ++k)
        if (finite[k] && finite[k + 1] && neg[k] != neg[k + 1]) {
            Bracket b;
            b.a = E[k]; b.b = E[k + 1]; b.neg_a = neg[k] != 0;
            out.push_back(b);
        }
    return out;
}

bool cut_bracket(Bracket* br, const double* E, const unsigned char* finite, const unsigned char* neg)
{
    bool bad = false;
    for (int j = 0; j < kCuts; ++j) bad = bad || !finite[j];       // any of the 64 cuts, also those above the pair picked below
    double pa = br->a;
    for (int j = 0; j <= kCuts; ++j) {               // the pair (p_j, p_j+1) of a, the cuts, b
        const bool last = j == kCuts;
        bool ng = !br->neg_a;                        // b's
        if (!last) ng = finite[j] ? neg[j] != 0 : br->neg_a;
        const double pb = last ? br->b : E[j];
        if (ng != br->neg_a) {
            br->a = pa; br->b = pb;
            break;
        }
        pa = pb;
    }
    return bad;
}

int search(const std::vector<SearchChannel>& ch, int nscan, const Evaluate& evaluate, SearchResult* out)
{
    const int nch = (int)ch.size();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    out->count.assign(nch, 0); out->rounds.assign(nch, 0); out->status.assign(nch, 0);
    out->energies.assign((size_t)nch * kMaxStates, nan);
    std::vector<int> tc, tm, st;
    std::vector<double> tE, u;
    std::vector<unsigned char> fin, neg;
    auto run = [&]() -> int {
        if (const int rc = evaluate(tc, tE, tm, &u, &st)) return rc;
        fin.resize(tE.size()); neg.resize(tE.size());
        for (size_t t = 0; t < tE.size(); ++t) {
            fin[t] = st[t] == 0 && std::isfinite(u[t]);
            neg[t] = u[t] < 0.;
        }
        return DFTA_OK;
    };
    // round 0
    for (int k = 0; k < nch; ++k)
        for (int j = 0; j < nscan; ++j) { tc.push_back(k); tE.push_back(scan_energy(ch[k].lo, ch[k].hi, nscan, j)); tm.push_back(ch[k].m); }
    if (const int rc = run()) return rc;
    std::vector<std::vector<Bracket>> br((size_t)nch);
    for (int k = 0; k < nch; ++k) {
        const size_t at = (size_t)k * nscan;
        br[k] = open_brackets(nscan, &tE[at], &fin[at], &neg[at]);
        out->rounds[k] = 1;
        int changes = 0;
        for (int j = 0; j + 1 < nscan; ++j) changes += fin[at + j] && fin[at + j + 1] && neg[at + j] != neg[at + j + 1];
        if (changes > kMaxStates) out->status[k] |= DFTA_KB_SEARCH_FULL;
    }
    // further rounds: every open bracket of every channel, one wave each, one launch
    for (int round = 1; round <= kMaxRounds; ++round) {
        tc.clear(); tE.clear(); tm.clear();
        std::vector<std::pair<int, int>> open;
        for (int k = 0; k < nch; ++k)
            for (size_t q = 0; q < br[k].size(); ++q)
                if (!bracket_closed(br[k][q].a, br[k][q].b)) {
                    open.emplace_back(k, (int)q);
                    for (int j = 0; j < kCuts; ++j) { tc.push_back(k); tE.push_back(cut_energy(br[k][q].a, br[k][q].b, j)); tm.push_back(ch[k].m); }
                }
        if (open.empty()) break;
        if (round == kMaxRounds) {
            for (const auto& o : open) out->status[o.first] |= DFTA_KB_SEARCH_CAP;
            break;
        }
        if (const int rc = run()) return rc;
        for (size_t o = 0; o < open.size(); ++o) {
            const int k = open[o].first;
            const size_t at = o * kCuts;
            if (cut_bracket(&br[k][open[o].second], &tE[at], &fin[at], &neg[at])) out->status[k] |= DFTA_KB_SEARCH_NONFINITE;
            out->rounds[k] = round + 1;
        }
    }
    for (int k = 0; k < nch; ++k) {
        out->count[k] = (int)br[k].size();
        for (size_t q = 0; q < br[k].size(); ++q) out->energies[(size_t)k * kMaxStates + q] = br[k][q].a;
    }
    return DFTA_OK;
}

}  // namespace dfta_kb_plan
