// Stand-in for <BipedalLocomotion/Contacts/ContactPhaseList.h> (and Contact.h / ContactList.h it pulls in): the
// members the reference touches on the CentroidalMPC path.  See ../../README.md.
//   PlannedContact: pose, activationTime, deactivationTime, name, index        CentroidalMPCBlock.cpp:79-81, :350-360
//   ContactList: addContact, getNextContact, getActiveContact, cbegin / cend   CentroidalMPCBlock.cpp:44-48, :61, :69
//                (an ordered set: its iterators are bidirectional, not random access)
//   ContactList / ContactPhaseList: forceSampleTime(dT)                        CentroidalMPCBlock.cpp:588
//   ContactPhaseList: lists(), setLists()                                      CentroidalMPCBlock.cpp:41, :60, :107
//   DiscreteGeometryContact: pose, corners[].position / .force, name, index    WholeBodyQPBlock.cpp:824-829, :1319-1335
#pragma once
#include <chrono>
#include <map>
#include <set>
#include <string>
#include <vector>

#include <manif/manif.h>

namespace BipedalLocomotion {
namespace Contacts {

struct ContactBase {
    manif::SE3d pose;
    int index{-1};
    std::string name;
};
struct PlannedContact : public ContactBase {
    std::chrono::nanoseconds activationTime{std::chrono::nanoseconds::zero()};
    std::chrono::nanoseconds deactivationTime{std::chrono::nanoseconds::max()};
};
struct Corner {
    Eigen::Vector3d position;
    Eigen::Vector3d force;
};
struct DiscreteGeometryContact : public ContactBase {
    std::vector<Corner> corners;
};

class ContactList {
    struct Before {
        bool operator()(const PlannedContact& a, const PlannedContact& b) const { return a.deactivationTime <= b.activationTime; }
    };
    std::set<PlannedContact, Before> m_contacts;  // ordered by time, contacts of one foot do not overlap
    static constexpr long long kNever = 1000000000LL * 1000000000LL;   // 1e9 s
    static long long snap(long long t, long long dt)
    {
        if (t >= kNever || t <= -kNever || t % dt == 0) return t;
        const long long num = 2 * t + dt, den = 2 * dt;
        long long q = num / den;
        if (num % den != 0 && num < 0) --q;   // floor division
        return q * dt;
    }
public:
    using const_iterator = std::set<PlannedContact, Before>::const_iterator;
    bool addContact(const PlannedContact& c)
    {
        if (c.deactivationTime < c.activationTime) return false;
        return m_contacts.insert(c).second;  // an overlapping contact compares equivalent: refused, as in BLF
    }
    const_iterator cbegin() const { return m_contacts.cbegin(); }
    const_iterator cend() const { return m_contacts.cend(); }
    const_iterator begin() const { return m_contacts.cbegin(); }
    const_iterator end() const { return m_contacts.cend(); }
    std::size_t size() const { return m_contacts.size(); }
    // the contact with activationTime <= t < deactivationTime, or cend()
    const_iterator getActiveContact(const std::chrono::nanoseconds& t) const
    {
        for (auto it = m_contacts.cbegin(); it != m_contacts.cend(); ++it)
            if (it->activationTime <= t && t < it->deactivationTime) return it;
        return m_contacts.cend();
    }
    // every activation / deactivation time to the nearest multiple of dT counted from time 0, ties to the later one; |t| >= 1e9 s (the "never"
    // of an open-ended contact) is kept.  BLF's own rule is not in the reference tree: this is the rule of include/cmpc.h
    // (cmpc_contacts_force_sample_time), on the same integer nanoseconds.  false -- the list left as it was -- if dT <= 0 or a contact of positive
    // duration would collapse to zero duration.
    bool forceSampleTime(const std::chrono::nanoseconds& dT)
    {
        const long long dt = dT.count();
        if (dt <= 0 || dt >= kNever) return false;
        std::set<PlannedContact, Before> snapped;
        for (const PlannedContact& c : m_contacts) {
            PlannedContact s = c;
            s.activationTime = std::chrono::nanoseconds(snap(c.activationTime.count(), dt));
            s.deactivationTime = std::chrono::nanoseconds(snap(c.deactivationTime.count(), dt));
            if (c.deactivationTime > c.activationTime && s.deactivationTime == s.activationTime) return false;
            if (!snapped.insert(s).second) return false;   // (cannot happen: the rounding is monotone, order and non-overlap are kept)
        }
        m_contacts.swap(snapped);
        return true;
    }
    // the contact with the lowest activationTime strictly after t, or cend()
    const_iterator getNextContact(const std::chrono::nanoseconds& t) const
    {
        for (auto it = m_contacts.cbegin(); it != m_contacts.cend(); ++it)
            if (it->activationTime > t) return it;
        return m_contacts.cend();
    }
};
using ContactListMap = std::map<std::string, ContactList>;

class ContactPhaseList {
    ContactListMap m_lists;
public:
    const ContactListMap& lists() const { return m_lists; }
    bool setLists(const ContactListMap& l) { m_lists = l; return true; }
    // every list's ContactList::forceSampleTime; false -- every list left as it was -- if one of them fails
    bool forceSampleTime(const std::chrono::nanoseconds& dT)
    {
        ContactListMap snapped = m_lists;
        for (auto& kv : snapped)
            if (!kv.second.forceSampleTime(dT)) return false;
        m_lists.swap(snapped);
        return true;
    }
};

}  // namespace Contacts
}  // namespace BipedalLocomotion
