// FSI coupling driver on the MI355X path: a test harness for the facade's matched interface, not a product.  One rank.
//   Domain::buildMesh on the unit square / cube                                              (the generator of both sides)
//   -> the FLUID domain: that mesh, the nodes on x = 1 re-flagged to the interface flag(s)
//   -> the STRUCTURE domain: the same mesh shifted by +1 in x, the nodes on x = 1 (its side x = 0 before the shift) put on
//      x = 1.0 exactly and re-flagged alike.  Both through Domain::setMesh, the entry for externally built meshes.
//      With two flags the interface nodes with y < 0.5 carry the smaller one and the others the larger one.
//   -> fluid->identifyInterfaceParallelAndDistance(structure, flags), structure->identifyInterfaceParallelAndDistance(fluid, flags)
//      (the two calls of the reference's FSI main: the second reads the table the first one left)
//   -> with --partial=FLAG:TYPE, setPartialCoupling(FLAG, TYPE) on both
//   -> on stdout, for each side S in {fluid, structure}:
//        node S <local unique id> <global id> <x> <y> [<z>]
//        matched S <flag index> <flag> <j> <global id of this side> <global id of the other side>      getIndicesGlobalMatched
//        map S <name> <i> <global element i>        the interface maps, name = interface | interfaceVec | global | globalVec |
//                                                   otherGlobal | otherGlobalVec | partialVec | otherPartialVec
//        mask S <k> <0 | 1>                         interfaceCoupledMask
//        local S <k> <local unique node id of pair k>
//      and "pairs <n> max_distance <d> fluid_side <0 | 1> <0 | 1>" from fedd_interface_match_info and the two domains.
// Options: --dim=2|3  --fe=P1|P2  --m=<cells per direction>  --flag=<N> (may repeat, at most two)  --partial=<FLAG>:<TYPE>
#include <cmath>
#include <cstdlib>
#include <iomanip>
#include <iostream>

#include "feddlib/core/FEDDCore.hpp"
#include "feddlib/core/FE/Domain.hpp"

typedef default_sc SC;
typedef default_lo LO;
typedef default_go GO;
typedef default_no NO;
using namespace FEDD;
typedef Domain<SC, LO, GO, NO> Domain_Type;
typedef Teuchos::RCP<Domain_Type> DomainPtr_Type;

static DomainPtr_Type side(const DomainPtr_Type& base, double shift, const std::vector<int>& flags) {
    const int dim = (int)base->getDimension();
    std::vector<double> xyz = base->xyzRepeated();
    for (size_t i = 0; i < xyz.size() / dim; ++i) {
        xyz[i * dim] += shift;
        if (std::fabs(xyz[i * dim] - 1.0) < 1e-12) xyz[i * dim] = 1.0;
    }
    const std::vector<int32_t>& repOfUni = base->uniqueLocalOfRepeated();
    vec_int_ptr_Type flagBase = base->getBCFlagUnique();
    std::vector<int32_t> flagUni(flagBase->begin(), flagBase->end());
    const int lo = *std::min_element(flags.begin(), flags.end()), hi = *std::max_element(flags.begin(), flags.end());
    for (size_t i = 0; i < flagUni.size(); ++i) {
        const double* p = &xyz[(size_t)repOfUni[i] * dim];
        if (p[0] == 1.0) flagUni[i] = p[1] < 0.5 ? lo : hi;
    }
    std::vector<int64_t> gidRep(base->getMapRepeated()->gids().begin(), base->getMapRepeated()->gids().end());
    std::vector<int64_t> gidUni(base->getMapUnique()->gids().begin(), base->getMapUnique()->gids().end());
    DomainPtr_Type d(new Domain_Type(base->getComm(), dim));
    d->setMesh(dim, base->getFEType(), base->nodesPerElement(), base->connectivity(), xyz, gidRep, gidUni, flagUni);
    return d;
}

static void printMap(const char* who, const char* name, const Domain_Type::MapConstPtr_Type& map) {
    if (map.is_null()) return;
    for (LO i = 0; i < map->getNodeNumElements(); ++i) std::cout << "map " << who << " " << name << " " << i << " " << map->getGlobalElement(i) << "\n";
}

static void print(const char* who, const DomainPtr_Type& d, const std::vector<int>& flags) {
    const int dim = (int)d->getDimension();
    vec2D_dbl_ptr_Type pts = d->getPointsUniqueRef();
    for (size_t i = 0; i < pts->size(); ++i) {
        std::cout << "node " << who << " " << i << " " << d->getMapUnique()->getGlobalElement((LO)i);
        for (int k = 0; k < dim; ++k) std::cout << " " << (*pts)[i][k];
        std::cout << "\n";
    }
    vec3D_GO_ptr_Type matched = d->getIndicesGlobalMatched();
    for (size_t q = 0; q < matched->size(); ++q)
        for (size_t j = 0; j < (*matched)[q][0].size(); ++j)
            std::cout << "matched " << who << " " << q << " " << flags[q] << " " << j << " " << (*matched)[q][0][j] << " " << (*matched)[q][1][j] << "\n";
    printMap(who, "interface", d->getInterfaceMapUnique());
    printMap(who, "interfaceVec", d->getInterfaceMapVecFieldUnique());
    printMap(who, "global", d->getGlobalInterfaceMapUnique());
    printMap(who, "globalVec", d->getGlobalInterfaceMapVecFieldUnique());
    printMap(who, "otherGlobal", d->getOtherGlobalInterfaceMapUnique());
    printMap(who, "otherGlobalVec", d->getOtherGlobalInterfaceMapVecFieldUnique());
    printMap(who, "partialVec", d->getGlobalInterfaceMapVecFieldPartial());
    printMap(who, "otherPartialVec", d->getOtherGlobalInterfaceMapVecFieldPartial());
    const std::vector<uint8_t>& mask = d->interfaceCoupledMask();
    for (size_t k = 0; k < mask.size(); ++k) std::cout << "mask " << who << " " << k << " " << (int)mask[k] << "\n";
    const std::vector<int32_t>& loc = d->interfaceNodesLocal();
    for (size_t k = 0; k < loc.size(); ++k) std::cout << "local " << who << " " << k << " " << loc[k] << "\n";
}

int main(int argc, char* argv[]) {
    Teuchos::GlobalMPISession mpiSession(&argc, &argv);
    int dim = 2, m = 4, partialFlag = 0;
    std::string fe = "P2", partialType;
    std::vector<int> flags;
    for (int i = 1; i < argc; ++i) {
        const std::string a(argv[i]);
        auto val = [&](const char* key, std::string& dst) {
            const std::string k = std::string("--") + key + "=";
            if (a.compare(0, k.size(), k) == 0) { dst = a.substr(k.size()); return true; }
            return false;
        };
        std::string t;
        if (val("dim", t)) { dim = std::atoi(t.c_str()); continue; }
        if (val("m", t)) { m = std::atoi(t.c_str()); continue; }
        if (val("fe", fe)) continue;
        if (val("flag", t)) { flags.push_back(std::atoi(t.c_str())); continue; }
        if (val("partial", t)) {
            const size_t c = t.find(':');
            if (c == std::string::npos) { std::cerr << "--partial wants FLAG:TYPE" << std::endl; return 2; }
            partialFlag = std::atoi(t.substr(0, c).c_str());
            partialType = t.substr(c + 1);
            continue;
        }
        std::cerr << "unknown option " << a << std::endl;
        return 2;
    }
    if (flags.empty()) flags.push_back(7);
    if (flags.size() > 2 || (dim != 2 && dim != 3) || m < 1) { std::cerr << "--dim=2|3, --m >= 1, at most two --flag" << std::endl; return 2; }
    try {
        Teuchos::RCP<const Teuchos::Comm<int> > comm = Teuchos::DefaultComm<int>::getComm();
        TEUCHOS_TEST_FOR_EXCEPTION(comm->getSize() != 1, std::logic_error, "fsicoupling driver: one rank");
        std::vector<double> x((size_t)dim, 0.0);
        DomainPtr_Type base = dim == 2 ? Teuchos::rcp(new Domain_Type(x, 1., 1., comm)) : Teuchos::rcp(new Domain_Type(x, 1., 1., 1., comm));
        base->buildMesh(1, "Square", dim, fe, 1, m, 0);
        DomainPtr_Type fluid = side(base, 0.0, flags), structure = side(base, 1.0, flags);

        fluid->identifyInterfaceParallelAndDistance(structure, flags);
        structure->identifyInterfaceParallelAndDistance(fluid, flags);
        if (!partialType.empty()) {
            fluid->setPartialCoupling(partialFlag, partialType);
            structure->setPartialCoupling(partialFlag, partialType);
        }
        std::cout << std::setprecision(17);
        print("fluid", fluid, flags);
        print("structure", structure, flags);
        int have = 0;
        int64_t nPairs = 0;
        double maxDist = 0.;
        feddCheck(fedd_interface_match_info(fluid->device()->ctx, &have, &nPairs, &maxDist, nullptr), "fedd_interface_match_info");
        TEUCHOS_TEST_FOR_EXCEPTION(!have, std::logic_error, "the fluid's context holds no matched interface");
        std::cout << "pairs " << nPairs << " max_distance " << maxDist << " fluid_side " << fluid->isFluidSideOfMatch() << " "
                  << structure->isFluidSideOfMatch() << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
