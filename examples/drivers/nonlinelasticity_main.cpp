// Nonlinear elasticity driver on the MI355X path, written against the FEDD:: operator surface the way the reference's test is
// (feddlib/problems/tests/nonLinElasticity/main.cpp:142-321): same XML parameter files, same call sequence
//   Domain::buildMesh (unit square / cube) | MeshPartitioner::readAndPartition -> BCBuilder::addBC(zero Dirichlet on flag 2,
//   unstructured: 1) -> NonLinElasticity(...) -> addBoundaries -> addRhsFunction(rhs2D | rhsX) -> addParemeterRhs(force, degree)
//   -> initializeProblem -> assemble -> setBoundaries -> NonLinearSolver("Linearization")::solve -> export.
// "Discretization" = "P2" on a structured mesh: the P2 mesh of the structured P1 mesh (the structured generator of this build
// makes P1 meshes).  Output: the reference's iteration lines on stdout, the displacement as text.
#include <cmath>
#include <fstream>
#include <iomanip>

#include "feddlib/core/FEDDCore.hpp"
#include "feddlib/core/FE/Domain.hpp"
#include "feddlib/core/Mesh/MeshPartitioner.hpp"
#include "feddlib/core/General/BCBuilder.hpp"
#include "feddlib/core/General/ExporterParaView.hpp"
#include "feddlib/problems/specific/NonLinElasticity.hpp"
#include "feddlib/problems/Solver/NonLinearSolver.hpp"

// parameters[0] is the time, parameters[1] the volume force
void rhs2D(double* x, double* res, double* parameters) { res[0] = 0.; res[1] = parameters[1]; }
void rhsX(double* x, double* res, double* parameters) { res[0] = parameters[1]; res[1] = 0.; res[2] = 0.; }
void zeroDirichlet2D(double* x, double* res, double t, const double* parameters) { res[0] = 0.; res[1] = 0.; }
void zeroDirichlet3D(double* x, double* res, double t, const double* parameters) { res[0] = 0.; res[1] = 0.; res[2] = 0.; }

typedef default_sc SC;
typedef default_lo LO;
typedef default_go GO;
typedef default_no NO;

using namespace FEDD;

int main(int argc, char* argv[]) {
    typedef Teuchos::RCP<Domain<SC, LO, GO, NO> > DomainPtr_Type;
    std::string xmlProblemFile = "parametersProblem.xml", xmlPrecFile = "parametersPrec.xml", xmlSolverFile = "parametersSolver.xml";
    std::string outFile = "solutionNonLinElasticity.txt";
    for (int i = 1; i < argc; ++i) {
        std::string a(argv[i]);
        auto val = [&](const char* key, std::string& dst) {
            const std::string k = std::string("--") + key + "=";
            if (a.compare(0, k.size(), k) == 0) { dst = a.substr(k.size()); return true; }
            return false;
        };
        if (val("problemfile", xmlProblemFile) || val("precfile", xmlPrecFile) || val("solverfile", xmlSolverFile) || val("out", outFile)) continue;
        std::cerr << "unknown option " << a << std::endl;
        return 2;
    }
    try {
        Teuchos::RCP<const Teuchos::Comm<int> > comm = Teuchos::rcp(new Teuchos::Comm<int>(0, 1));
        ParameterListPtr_Type parameterListProblem = Teuchos::getParametersFromXmlFile(xmlProblemFile);
        ParameterListPtr_Type parameterListPrec = Teuchos::getParametersFromXmlFile(xmlPrecFile);
        ParameterListPtr_Type parameterListSolver = Teuchos::getParametersFromXmlFile(xmlSolverFile);

        int dim = parameterListProblem->sublist("Parameter").get("Dimension", 3);
        std::string meshType = parameterListProblem->sublist("Parameter").get("Mesh Type", "structured");
        int m = parameterListProblem->sublist("Parameter").get("H/h", 5);
        int volumeID = parameterListProblem->sublist("Parameter").get("Volume ID", 10);
        std::string FEType = parameterListProblem->sublist("Parameter").get("Discretization", "P1");
        TEUCHOS_TEST_FOR_EXCEPTION(FEType != "P1" && FEType != "P2", std::logic_error, "Discretization: P1 and P2 are built");

        ParameterListPtr_Type parameterListAll(new Teuchos::ParameterList(*parameterListProblem));
        parameterListAll->setParameters(*parameterListPrec);
        parameterListAll->setParameters(*parameterListSolver);

        if (comm->getRank() == 0) {
            std::cout << "######################################" << std::endl;
            std::cout << "########## Nonlinear Elasticity ######" << std::endl;
            std::cout << "######################################" << std::endl;
        }
        DomainPtr_Type domainP1, domain;
        if (meshType == "structured") {
            if (dim == 2) {
                std::vector<double> x(2, 0.0);
                domainP1 = Teuchos::rcp(new Domain<SC, LO, GO, NO>(x, 1., 1., comm));
            } else {
                std::vector<double> x(3, 0.0);
                domainP1 = Teuchos::rcp(new Domain<SC, LO, GO, NO>(x, 1., 1., 1., comm));
            }
            domainP1->buildMesh(1, "Square", dim, "P1", 1, m, 0);
        } else if (meshType == "unstructured") {
            typedef MeshPartitioner<SC, LO, GO, NO> MeshPartitioner_Type;
            domainP1.reset(new Domain<SC, LO, GO, NO>(comm, dim));
            MeshPartitioner_Type::DomainPtrArray_Type domainP1Array(1);
            domainP1Array[0] = domainP1;
            ParameterListPtr_Type pListPartitioner = Teuchos::sublist(parameterListAll, "Mesh Partitioner");
            MeshPartitioner_Type partitionerP1(domainP1Array, pListPartitioner, "P1", dim);
            partitionerP1.readAndPartition(volumeID);
        } else {
            TEUCHOS_TEST_FOR_EXCEPTION(true, std::logic_error, "Mesh Type \"" + meshType + "\" is not built (structured, unstructured are)");
        }
        if (FEType == "P2") {
            domain.reset(new Domain<SC, LO, GO, NO>(comm, dim));
            domain->buildP2ofP1Domain(domainP1);
        } else {
            domain = domainP1;
        }

        Teuchos::RCP<BCBuilder<SC, LO, GO, NO> > bcFactory(new BCBuilder<SC, LO, GO, NO>());
        bcFactory->addBC(dim == 2 ? zeroDirichlet2D : zeroDirichlet3D, meshType == "structured" ? 2 : 1, 0, domain, "Dirichlet", dim);

        NonLinElasticity<SC, LO, GO, NO> elasticity(domain, FEType, parameterListAll);
        domain->info();
        elasticity.info();
        {
            elasticity.addBoundaries(bcFactory);
            elasticity.addRhsFunction(dim == 2 ? rhs2D : rhsX);
            double force = parameterListAll->sublist("Parameter").get("Volume force", 0.);
            double degree = 0;
            elasticity.addParemeterRhs(force);
            elasticity.addParemeterRhs(degree);
            elasticity.initializeProblem();
            elasticity.assemble();
            elasticity.setBoundaries();
            std::string nlSolverType = parameterListProblem->sublist("General").get("Linearization", "Newton");
            NonLinearSolver<SC, LO, GO, NO> elasticitySolver(nlSolverType);
            elasticitySolver.solve(elasticity);
        }
        Teuchos::RCP<const MultiVector<SC, LO, GO, NO> > exportSolutionU = elasticity.getSolution()->getBlock(0);
        std::ofstream out(outFile);
        out << std::setprecision(17);
        auto map = exportSolutionU->getMap();
        auto data = exportSolutionU->getData(0);
        for (size_t i = 0; i < data.size(); ++i) out << map->getGlobalElement((LO)i) << " " << data[i] << "\n";
        if (parameterListAll->sublist("General").get("ParaViewExport", false)) {
            Teuchos::RCP<ExporterParaView<SC, LO, GO, NO> > exParaDisp(new ExporterParaView<SC, LO, GO, NO>());
            exParaDisp->setup("displacement", domain->getMesh(), domain->getFEType());
            exParaDisp->addVariable(exportSolutionU, "u", "Vector", dim, domain->getMapUnique());
            exParaDisp->save(0.0);
        }
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
