// Drives gorder_amd/csrc/switches.h without a device (built with -fsanitize=address,undefined by
// tests/test_switches_cpu.py, which holds the expected values).
//
//   switches                   the table: one line "NAME<tab>meaning" per switch, in kSwitches' order
//   switches NAME=VALUE ...    read_switches over that environment (a name not given is not set): one line
//                              "member value" per member of gorder::Switches, in the struct's order, then one line
//                              "lookup NAME count" per name read_switches asked for
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "switches.h"

int main(int argc, char **argv) {
    if (argc == 1) {
        for (const gorder::Switch &w : gorder::kSwitches) printf("%s\t%s\n", w.name, w.meaning);
        return 0;
    }
    std::map<std::string, std::string> env;
    for (int i = 1; i < argc; i++) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "%s: not NAME=VALUE\n", argv[i]); return 2; }
        env[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
    }
    std::vector<std::string> asked;
    const gorder::Switches s = gorder::read_switches([&](const char *name) -> const char * {
        asked.push_back(name);
        const auto at = env.find(name);
        return at == env.end() ? nullptr : at->second.c_str();
    });
    const auto put = [](const char *member, unsigned long long v) { printf("%s %llu\n", member, v); };
#define PUT(member) put(#member, (unsigned long long)s.member)
    PUT(kernel_gather); PUT(wg_target); PUT(npf5); PUT(tw_gather); PUT(maps_gather); PUT(force_direct); PUT(ua_slot_waves); PUT(replicas);
    PUT(map_direct); PUT(map_chunks);
    printf("map_fold_limit %ld\n", s.map_fold_limit);       // (signed: the value as written)
    PUT(no_speculate); PUT(leaflets_generic); PUT(spherical_slab); PUT(cluster_stored_w); PUT(local_slab); PUT(local_atoms_only);
    PUT(local_three_kernels); PUT(local_no_decide); PUT(local_no_sums); PUT(local_no_prune); PUT(local_decide_nothing);
    PUT(radial_direct); PUT(dist_direct); PUT(dist_samples_per_word); PUT(nb_direct); PUT(nb_subrange); PUT(nb_row_bytes);
    PUT(corr_subrange); PUT(corr_grid_chunks); PUT(mol_rows_staging);
    PUT(prefix_q16); PUT(no_prefix);
#undef PUT
    std::map<std::string, int> count;
    for (const std::string &name : asked) count[name]++;
    for (const auto &c : count) printf("lookup %s %d\n", c.first.c_str(), c.second);
    return 0;
}
