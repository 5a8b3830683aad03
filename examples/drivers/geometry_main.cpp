// Geometry driver on the MI355X path: the fluid half of the reference's geometry test
// (feddlib/problems/tests/geometry/main.cpp:436-700) on ONE domain, written against the FEDD:: operator surface with the
// reference's three XML parameter files:
//   Domain::buildMesh -> BCBuilder::addBC (zero Dirichlet on the outer flags 1 and 2, a prescribed displacement on "Moving Flag")
//   -> with --interface-flag=N (may repeat): Domain::identifyInterfaceParallelAndDistance(domain, {N, ...}) on the driver's own
//      domain, which gives it the distances the default model "Laplace" of Geometry needs (without the option nothing changes)
//   -> Geometry(...) -> initializeProblem -> assemble -> setBoundaries -> solve          (the extension d_f of the displacement)
//   -> the repeated displacement from the unique solution -> Domain::moveMesh(d_unique, d_repeated)      (main.cpp:683)
//   -> Laplace(...) on the MOVED domain: assemble -> setBoundaries -> solve.
// Out of scope, unlike the reference driver: the structure mesh and its problem, the matching of the two interfaces (the
// displacement on "Moving Flag" is a constant vector from the problem file instead of the structure's solution), the
// unstructured meshes of the FSI benchmark (a structured square / cube is built), the subdomain exports, more than one rank.
// Output: <out>.d.txt (the extension, by global dof id), <out>.u.txt (the Laplace solution on the moved mesh, by global node
// id), <out>.xyz.txt (the moved repeated points, read back from the device), and on stdout the iteration counts, n_moves,
// min_det_ratio and the launches of the symbolic timer before the move and after the move and the assembly that follows it.
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>

#include "feddlib/core/FEDDCore.hpp"
#include "feddlib/core/FE/Domain.hpp"
#include "feddlib/core/General/BCBuilder.hpp"
#include "feddlib/problems/specific/Geometry.hpp"
#include "feddlib/problems/specific/Laplace.hpp"

static double g_disp[3] = {0., 0., 0.};     // "Displacement X / Y / Z" of the problem file
void zeroBC(double* x, double* res, double t, const double* parameters) { res[0] = 0.; }
void zeroBC2D(double* x, double* res, double t, const double* parameters) { res[0] = 0.; res[1] = 0.; }
void zeroBC3D(double* x, double* res, double t, const double* parameters) { res[0] = 0.; res[1] = 0.; res[2] = 0.; }
void movedBC2D(double* x, double* res, double t, const double* parameters) { res[0] = g_disp[0]; res[1] = g_disp[1]; }
void movedBC3D(double* x, double* res, double t, const double* parameters) { res[0] = g_disp[0]; res[1] = g_disp[1]; res[2] = g_disp[2]; }
void oneFunc(double* x, double* res, double* parameters) { res[0] = 1.; }

typedef default_sc SC;
typedef default_lo LO;
typedef default_go GO;
typedef default_no NO;

using namespace FEDD;

static int64_t symbolicLaunches(fedd_ctx* ctx) {
    double ms = 0.;
    int64_t n = 0;
    feddCheck(fedd_timing_get(ctx, FEDD_T_SYMBOLIC, &ms, &n), "fedd_timing_get");
    return n;
}

static void writeByGlobalId(const std::string& file, const Teuchos::RCP<const MultiVector<SC, LO, GO, NO> >& v, int dofs) {
    std::ofstream out(file);
    out << std::setprecision(17);
    auto map = v->getMap();
    auto data = v->getData(0);
    for (size_t i = 0; i < data.size(); ++i) {
        // (a vector-field map lists dof ids already; a node map lists node ids)
        (void)dofs;
        out << map->getGlobalElement((LO)i) << " " << data[i] << "\n";
    }
}

int main(int argc, char* argv[]) {
    Teuchos::GlobalMPISession mpiSession(&argc, &argv);
    std::string xmlProblemFile = "parametersProblem.xml", xmlPrecFile = "parametersPrec.xml", xmlSolverFile = "parametersSolver.xml";
    std::string outFile = "geometry";
    std::vector<int> interfaceFlags;        // --interface-flag=N, may repeat
    for (int i = 1; i < argc; ++i) {
        std::string a(argv[i]);
        auto val = [&](const char* key, std::string& dst) {
            const std::string k = std::string("--") + key + "=";
            if (a.compare(0, k.size(), k) == 0) { dst = a.substr(k.size()); return true; }
            return false;
        };
        if (val("problemfile", xmlProblemFile) || val("precfile", xmlPrecFile) || val("solverfile", xmlSolverFile) || val("out", outFile)) continue;
        std::string flagText;
        if (val("interface-flag", flagText)) {
            char* end = nullptr;
            const long f = std::strtol(flagText.c_str(), &end, 10);
            if (flagText.empty() || *end != '\0') {
                std::cerr << "--interface-flag wants an integer, got \"" << flagText << "\"" << std::endl;
                return 2;
            }
            interfaceFlags.push_back((int)f);
            continue;
        }
        std::cerr << "unknown option " << a << std::endl;
        return 2;
    }
    try {
        Teuchos::RCP<const Teuchos::Comm<int> > comm = Teuchos::DefaultComm<int>::getComm();
        TEUCHOS_TEST_FOR_EXCEPTION(comm->getSize() != 1, std::logic_error, "geometry driver: one rank (Domain::moveMesh is one rank in this build)");
        ParameterListPtr_Type parameterListProblem = Teuchos::getParametersFromXmlFile(xmlProblemFile);
        ParameterListPtr_Type parameterListPrec = Teuchos::getParametersFromXmlFile(xmlPrecFile);
        ParameterListPtr_Type parameterListSolver = Teuchos::getParametersFromXmlFile(xmlSolverFile);
        ParameterListPtr_Type parameterListAll(new Teuchos::ParameterList(*parameterListProblem));
        parameterListAll->setParameters(*parameterListPrec);
        parameterListAll->setParameters(*parameterListSolver);

        auto& par = parameterListProblem->sublist("Parameter");
        const int dim = par.get("Dimension", 2);
        const int m = par.get("H/h", 10);
        const std::string discType = par.get("Discretization", "P2");
        const std::string meshType = par.get("Mesh Type", "unstructured");
        const int movingFlag = par.get("Moving Flag", 3);
        g_disp[0] = par.get("Displacement X", 0.);
        g_disp[1] = par.get("Displacement Y", 0.);
        g_disp[2] = par.get("Displacement Z", 0.);
        TEUCHOS_TEST_FOR_EXCEPTION(meshType != "structured", std::logic_error,
                                   "geometry driver: \"Mesh Type\" = \"" << meshType << "\": only \"structured\" is built here");

        // ---- 1. the mesh ----
        Teuchos::RCP<Domain<SC, LO, GO, NO> > domain;
        if (dim == 2) {
            std::vector<double> x(2, 0.0);
            domain = Teuchos::rcp(new Domain<SC, LO, GO, NO>(x, 1., 1., comm));
        } else {
            std::vector<double> x(3, 0.0);
            domain = Teuchos::rcp(new Domain<SC, LO, GO, NO>(x, 1., 1., 1., comm));
        }
        domain->buildMesh(1, "Square", dim, discType, 1, m, 0);
        fedd_ctx* ctx = domain->device()->ctx;
        fedd_timing_enable(ctx, 1);

        // ---- 2. boundary conditions of the extension ----
        Teuchos::RCP<BCBuilder<SC, LO, GO, NO> > bcGeometry(new BCBuilder<SC, LO, GO, NO>());
        for (int flag = 1; flag <= 3; ++flag) {
            if (flag == movingFlag) bcGeometry->addBC(dim == 2 ? movedBC2D : movedBC3D, flag, 0, domain, "Dirichlet", dim);
            else bcGeometry->addBC(dim == 2 ? zeroBC2D : zeroBC3D, flag, 0, domain, "Dirichlet", dim);
        }

        // ---- 2b. the interface and the distances to it (the driver has one domain: it is its own "other" side) ----
        if (!interfaceFlags.empty()) {
            domain->identifyInterfaceParallelAndDistance(domain, interfaceFlags);
            int have = 0;
            int64_t nInterface = 0;
            feddCheck(fedd_interface_distance_info(ctx, &have, &nInterface, nullptr), "fedd_interface_distance_info");
            std::cout << "interface nodes " << nInterface << std::endl;
        }

        // ---- 3. the extension ----
        Geometry<SC, LO, GO, NO> geometry(domain, discType, parameterListAll);
        geometry.addBoundaries(bcGeometry);
        geometry.initializeProblem();
        geometry.assemble();
        geometry.setBoundaries();
        const int itsGeometry = geometry.solve();
        std::cout << "geometry iterations " << itsGeometry << " relres " << geometry.getLastRelativeResidual() << std::endl;
        Teuchos::RCP<MultiVector<SC, LO, GO, NO> > dUnique = geometry.getSolution()->getBlockNonConst(0);

        // ---- 4. the repeated displacement, and the move ----
        Teuchos::RCP<MultiVector<SC, LO, GO, NO> > dRepeated(new MultiVector<SC, LO, GO, NO>(domain->getMapVecFieldRepeated()));
        {
            const auto& uniOfRep = domain->uniqueLocalOfRepeated();      // repeated-local id of every unique node
            const auto& du = dUnique->raw(0);
            auto& dr = dRepeated->raw(0);
            for (size_t i = 0; i < uniOfRep.size(); ++i)
                for (int k = 0; k < dim; ++k) dr[(size_t)uniOfRep[i] * dim + k] = du[i * dim + k];
        }
        const int64_t symbolicBefore = symbolicLaunches(ctx);
        domain->moveMesh(dUnique, dRepeated);
        int64_t nMoves = 0, geometryId = 0;
        double minDetRatio = 0.;
        feddCheck(fedd_mesh_move_info(ctx, &nMoves, &geometryId, &minDetRatio), "fedd_mesh_move_info");

        // the extension once more on the moved mesh (what the next step of an ALE loop does): its pattern, the adjacency and the
        // tile structures stand, so neither the move nor this assembly may count a launch of the symbolic timer
        geometry.assemble();
        geometry.setBoundaries();
        const int64_t symbolicAfter = symbolicLaunches(ctx);

        // ---- 5. a Laplace problem on the moved domain (another pattern in the same context: its build is a build) ----
        Teuchos::RCP<BCBuilder<SC, LO, GO, NO> > bcLaplace(new BCBuilder<SC, LO, GO, NO>());
        for (int flag = 1; flag <= 3; ++flag) bcLaplace->addBC(zeroBC, flag, 0, domain, "Dirichlet", 1);
        Laplace<SC, LO, GO, NO> laplace(domain, discType, parameterListAll, false);
        laplace.addRhsFunction(oneFunc);
        laplace.addBoundaries(bcLaplace);
        laplace.initializeProblem();
        laplace.assemble();
        laplace.setBoundaries();
        const int itsLaplace = laplace.solve();
        std::cout << "laplace iterations " << itsLaplace << " relres " << laplace.getLastRelativeResidual() << std::endl;

        // ---- 6. the results ----
        writeByGlobalId(outFile + ".d.txt", dUnique, dim);
        writeByGlobalId(outFile + ".u.txt", laplace.getSolution()->getBlock(0), 1);
        {
            std::vector<double> xyz(domain->xyzRepeated().size());
            feddCheck(fedd_mesh_coords_get(ctx, xyz.data()), "fedd_mesh_coords_get");
            std::ofstream out(outFile + ".xyz.txt");
            out << std::setprecision(17);
            auto map = domain->getMapRepeated();
            for (size_t i = 0; i < xyz.size() / dim; ++i) {
                out << map->getGlobalElement((LO)i);
                for (int k = 0; k < dim; ++k) out << " " << xyz[i * dim + k];
                out << "\n";
            }
            TEUCHOS_TEST_FOR_EXCEPTION(xyz != domain->xyzRepeated(), std::logic_error, "the device's points differ from the domain's");
        }
        // ---- 7. the move in numbers ----
        std::cout << "n_moves " << nMoves << " geometry_id " << geometryId << " min_det_ratio " << std::setprecision(17) << minDetRatio << std::endl;
        std::cout << "symbolic launches before move " << symbolicBefore << " after move " << symbolicAfter << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
