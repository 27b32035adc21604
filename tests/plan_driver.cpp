// The call plan on the CPU: reads cases from stdin, one per line, builds the FitPlan of each (insider_plan.hpp) and prints
// every field of it, one line per case.  tests/test_plan_cpu.py compares the answers with the hand-written rules of
// tests/dispatch_rules.py.  Includes the shapes header and the plan header only: no HIP, no handle, no device.
//
// A case is a list of name=value tokens.  Names: the integer members of PlanFacts; "opt.<name>" for its options; "L",
// "npairs", "cf_L", "cf_nlater" take comma-separated lists; "masked"; "alpha" and "la" (both given: the call runs a column
// solve); "sites" = M:L,M:L,... asks reduce_form() at each launch site and "vn" = N,N,... mm_rows_nt(); "batch" = 1 asks
// cd_solver() as the batch entry does (default options).  An unknown name is an error: no case is read half.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../insider_amd/csrc/insider_shapes.hpp"
#include "../insider_amd/csrc/insider_plan.hpp"

namespace {

std::vector<long long> int_list(const std::string &v)
{
    std::vector<long long> out;
    std::stringstream ss(v);
    std::string item;
    while (std::getline(ss, item, ',')) out.push_back(std::stoll(item));
    return out;
}

struct Case {
    PlanFacts f;
    int masked = 1, batch = 0;
    bool has_alpha = false, has_la = false;
    ColCall col{0.0, 0.0};
    std::vector<std::pair<long long, int>> sites;
    std::vector<int> vn;
};

bool set_field(Case &c, const std::string &k, const std::string &v)
{
    PlanFacts &f = c.f;
#define INT_FIELD(name, member) if (k == name) { member = static_cast<decltype(member)>(std::stoll(v)); return true; }
#define FACT(n) INT_FIELD(#n, f.n)
#define OPT(n) INT_FIELD("opt." #n, f.opt.n)
    OPT(row_merged) OPT(col_factored) OPT(row_fused) OPT(row_gemm) OPT(row_counts) OPT(mm_fast) OPT(force_allreduce) OPT(wg_waves)
    OPT(list_fine) OPT(mm_tiles) OPT(col_mfma4) OPT(cd_variant) OPT(cd_pairs) OPT(cd_cold_iters) OPT(cd_pass_first)
    OPT(cd_pass_ratio) OPT(max_sweeps)
    FACT(world) FACT(n_simd) FACT(K) FACT(NB) FACT(KP) FACT(lvl_zero) FACT(fperm) FACT(merged) FACT(cont_merged)
    FACT(cf_pair_ok) FACT(cf_hn) FACT(cf_zt) FACT(c) FACT(m) FACT(SL) FACT(SLP) FACT(SLcat) FACT(n) FACT(p) FACT(col_entries)
    FACT(row_entries) FACT(cf_c) FACT(cf_tab_rows) FACT(cf_nsteps)
    INT_FIELD("masked", c.masked) INT_FIELD("batch", c.batch)
#undef OPT
#undef FACT
#undef INT_FIELD
    if (k == "alpha") { c.col.alpha = std::stod(v); return c.has_alpha = true; }
    if (k == "la") { c.col.la = std::stod(v); return c.has_la = true; }
    if (k == "L") { for (long long x : int_list(v)) f.L.push_back((int)x); return true; }
    if (k == "vn") { for (long long x : int_list(v)) c.vn.push_back((int)x); return true; }
    if (k == "npairs") { for (long long x : int_list(v)) f.npairs.push_back(x); return true; }
    if (k == "cf_L" || k == "cf_nlater") {
        const std::vector<long long> xs = int_list(v);
        if (xs.size() > (size_t)CF_MAXC + 1) return false;
        for (size_t t = 0; t < xs.size(); ++t) (k == "cf_L" ? f.cf_L : f.cf_nlater)[t] = (int)xs[t];
        return true;
    }
    if (k == "sites") {
        std::stringstream ss(v);
        std::string item;
        while (std::getline(ss, item, ',')) {
            const size_t colon = item.find(':');
            if (colon == std::string::npos) return false;
            c.sites.emplace_back(std::stoll(item.substr(0, colon)), std::stoi(item.substr(colon + 1)));
        }
        return true;
    }
    return false;
}

void print_plan(const Case &c, const FitPlan &p)
{
    std::ostringstream o;
    o << "masked=" << p.masked << " merged=" << p.merged << " unmasked_fused=" << p.unmasked_fused << " fused_solve=" << p.fused_solve
      << " row_fused=" << p.row_fused << " allreduce=" << p.allreduce << " list4=" << p.list4 << " mm_fast=" << p.mm_fast
      << " q_rows2=" << p.q_rows2 << " v_rows2=" << p.v_rows2 << " mm_tpw=" << p.mm_tpw << " col_path=" << p.col_path
      << " NB=" << p.NB << " KP=" << p.KP << " stat_len=" << p.stat_len << " plen=" << p.plen << " pc_kernel=" << (int)p.pc_kernel
      << " pc_lds=" << p.pc_lds << " pc_blocks=" << p.pc_blocks << " pc_parts=" << p.pc_parts << " col_solver=" << (int)p.col_solver
      << " col_eval=" << (int)p.col_eval << " ridge_fallback=" << p.ridge_fallback << " cold_iters=" << p.cold_iters
      << " npass=" << p.npass << " order_wide=" << p.order_wide << " order_pairs=" << p.order_pairs;
    o << " pass_limit=";
    for (int i = 0; i < p.npass; ++i) o << (i ? "," : "") << p.pass_limit[i];
    o << " wg=";
    for (size_t i = 0; i < p.wg.size(); ++i) {
        const WgPlan &w = p.wg[i];
        o << (i ? "," : "") << w.use << ':' << w.tiles << ':' << w.LT << ':' << w.zch << ':' << w.ntile << ':' << w.npair << ':'
          << w.slab << ':' << w.nslab;
    }
    o << " u_cnt=";
    for (size_t i = 0; i < p.u_cnt.size(); ++i) o << (i ? "," : "") << (int)p.u_cnt[i];
    o << " reduce=";
    for (size_t i = 0; i < c.sites.size(); ++i) o << (i ? "," : "") << (int)reduce_form(p, c.sites[i].first, c.sites[i].second);
    o << " v_nt=";
    for (size_t i = 0; i < c.vn.size(); ++i) o << (i ? "," : "") << mm_rows_nt(c.vn[i]);
    o << " batch_solver=" << (c.batch ? (int)cd_solver(c.f.K, c.col.la, 0) : -1);
    std::puts(o.str().c_str());
}

}  // namespace

int main()
{
    std::string line;
    long lineno = 0;
    while (std::getline(std::cin, line)) {
        ++lineno;
        if (line.empty()) continue;
        Case c;
        std::stringstream ss(line);
        std::string tok;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            bool ok = eq != std::string::npos;
            try {
                ok = ok && set_field(c, tok.substr(0, eq), tok.substr(eq + 1));
            } catch (const std::exception &) {
                ok = false;
            }
            if (!ok) {
                std::fprintf(stderr, "plan_driver: line %ld: bad token '%s'\n", lineno, tok.c_str());
                return 2;
            }
        }
        if (c.has_alpha != c.has_la || (int)c.f.L.size() != c.f.c || (!c.f.npairs.empty() && (int)c.f.npairs.size() != c.f.c)) {
            std::fprintf(stderr, "plan_driver: line %ld: alpha and la come together, L (and npairs) have c entries\n", lineno);
            return 2;
        }
        c.f.npairs.resize(c.f.c, 0);
        print_plan(c, build_plan(c.f, c.masked, c.has_alpha ? &c.col : nullptr));
    }
    return 0;
}
