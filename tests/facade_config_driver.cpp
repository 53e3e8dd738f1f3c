// Host-only driver of the C++ facade's initialize(): include/BipedalLocomotion/ReducedModelControllers/CentroidalMPC.h compiled against the
// csrc/shim/ headers, with stub definitions of the cmpc_* functions initialize() calls.  The stub cmpc_create records the cmpc_config the facade
// built and the driver prints it, so a CPU test can check what the class hands to the library for each shipped robot's ini file.
//
// argv[1]: parameters, one per line: "<group> <key> <type> <value...>" (group "-" is the top level; type i / d / b / s / v)
// argv[2]: the library's default tolerance per horizon, one "<N> <tolerance>" per line (written from the real library)
#include <BipedalLocomotion/ReducedModelControllers/CentroidalMPC.h>

#include <cstring>
#include <fstream>
#include <sstream>

namespace PH = BipedalLocomotion::ParametersHandler;

static cmpc_config g_seen;
static int g_created = 0;
static std::map<int, double> g_default_tol;

extern "C" {
void cmpc_default_config(cmpc_config* c) { std::memset(c, 0, sizeof(*c)); c->horizon = 20; c->sampling_time = 0.06; }
double cmpc_default_tolerance(int horizon) { return g_default_tol.at(horizon); }
int cmpc_create(const cmpc_config* cfg, int, int, cmpc_handle* out) { g_seen = *cfg; ++g_created; *out = (cmpc_handle)&g_seen; return CMPC_OK; }
int cmpc_destroy(cmpc_handle) { return CMPC_OK; }
const char* cmpc_last_error(cmpc_handle) { return ""; }
}

struct Handler : PH::IParametersHandler {
    struct V { char t; std::string s; std::vector<double> v; };
    std::map<std::string, V> kv;
    std::map<std::string, std::shared_ptr<Handler>> groups;
    const V* find(const std::string& k, const char* types) const
    {
        auto it = kv.find(k);
        return it != kv.end() && std::strchr(types, it->second.t) ? &it->second : nullptr;
    }
    bool getParameter(const std::string& k, int& x) const override { auto p = find(k, "i"); if (p) x = (int)p->v[0]; return p; }
    bool getParameter(const std::string& k, double& x) const override { auto p = find(k, "id"); if (p) x = p->v[0]; return p; }
    bool getParameter(const std::string& k, bool& x) const override { auto p = find(k, "b"); if (p) x = p->v[0] != 0; return p; }
    bool getParameter(const std::string& k, std::string& x) const override { auto p = find(k, "s"); if (p) x = p->s; return p; }
    bool getParameter(const std::string& k, std::vector<double>& x) const override { auto p = find(k, "v"); if (p) x = p->v; return p; }
    weak_ptr getGroup(const std::string& name) const override
    {
        auto it = groups.find(name);
        return it == groups.end() ? weak_ptr() : weak_ptr(it->second);
    }
};

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::ifstream tf(argv[2]);
    for (int n; tf >> n;) tf >> g_default_tol[n];
    auto root = std::make_shared<Handler>();
    std::ifstream pf(argv[1]);
    for (std::string line; std::getline(pf, line);) {
        std::istringstream is(line);
        std::string group, key;
        Handler::V v;
        if (!(is >> group >> key >> v.t)) continue;
        if (v.t == 's') is >> v.s;
        else for (double d; is >> d;) v.v.push_back(d);
        Handler* h = root.get();
        if (group != "-") {
            auto& g = root->groups[group];
            if (!g) g = std::make_shared<Handler>();
            h = g.get();
        }
        h->kv[key] = v;
    }
    BipedalLocomotion::ReducedModelControllers::CentroidalMPC mpc;
    if (!mpc.initialize(root) || g_created != 1) return 1;
    std::printf("horizon %d\ntolerance %.17g\nsampling_time %.17g\ncontact_position_weight %.17g\nmax_iterations %d\n",
                g_seen.horizon, g_seen.tolerance, g_seen.sampling_time, g_seen.contact_position_weight, g_seen.max_iterations);
    return 0;
}
