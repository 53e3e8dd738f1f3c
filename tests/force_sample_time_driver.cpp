// Host-only driver of the stand-in BipedalLocomotion::Contacts::ContactPhaseList::forceSampleTime (csrc/shim/), the call the reference makes at
// CentroidalMPCBlock.cpp:588, so that a CPU test can hold the shim's statement of the rule to the C ABI's (cmpc_contacts_force_sample_time).
//
// stdin:  "<dt_ns> <problems>", then per problem and foot (left_foot, right_foot): "<n> <activation_ns> <deactivation_ns> ..." (integer nanoseconds)
// stdout: per problem one line: "<ok> <n_left> <times...> <n_right> <times...>" -- the lists after the call (unchanged when it returns false);
//         ok = 2 when the input list could not be built (overlapping contacts)
#include <BipedalLocomotion/Contacts/ContactPhaseList.h>

#include <chrono>
#include <cstdio>
#include <iostream>

using namespace BipedalLocomotion::Contacts;

int main()
{
    long long dt_ns = 0;
    int problems = 0;
    if (!(std::cin >> dt_ns >> problems)) return 1;
    const char* names[2] = {"left_foot", "right_foot"};
    for (int p = 0; p < problems; ++p) {
        ContactListMap lists;
        bool built = true;
        for (const char* name : names) {
            int n = 0;
            std::cin >> n;
            ContactList& l = lists[name];
            for (int m = 0; m < n; ++m) {
                long long a = 0, d = 0;
                std::cin >> a >> d;
                PlannedContact c;
                c.name = name;
                c.index = m;
                c.activationTime = std::chrono::nanoseconds(a);
                c.deactivationTime = std::chrono::nanoseconds(d);
                built = l.addContact(c) && built;
            }
        }
        ContactPhaseList phase;
        phase.setLists(lists);
        const int ok = built ? (phase.forceSampleTime(std::chrono::nanoseconds(dt_ns)) ? 1 : 0) : 2;
        std::printf("%d", ok);
        for (const char* name : names) {
            const ContactList& l = phase.lists().at(name);
            std::printf(" %zu", l.size());
            for (const PlannedContact& c : l) std::printf(" %lld %lld", (long long)c.activationTime.count(), (long long)c.deactivationTime.count());
        }
        std::printf("\n");
    }
    return 0;
}
